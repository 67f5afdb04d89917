"""The intersection / PSDS scorer: DTC / GTC / CTTC counts on the GPU from the event lists of ``events``
(``intersection_counts_gpu``; rules as stated in include/bsed.h, parity with psds_eval not pinned), intersection F1, rates
and PSDS from the integer counts on the host (``intersection_f1``, ``psds_rates``, ``PsdsResult``)."""
import numpy as np
import torch

from .. import _lib as L
from .._lib import BsedError
from ._common import _accumulator, _host_counts, _macro_in_class_order


def _criteria(intersection, who):
    """``intersection`` argument of a scoring pass -> the ``(dtc, gtc, cttc)`` thresholds as floats (True = (0.5, 0.5,
    0.3)), or None for None and False: not asked for"""
    if intersection is None or intersection is False:
        return None
    if intersection is True:
        return 0.5, 0.5, 0.3
    try:
        dtc, gtc, cttc = (float(v) for v in intersection)
    except (TypeError, ValueError):
        raise BsedError(f"{who}: intersection must be None, True or a (dtc, gtc, cttc) tuple, got {intersection!r}") from None
    return dtc, gtc, cttc


def intersection_counts_gpu(events, reference, dtc=0.5, gtc=0.5, cttc=0.3, out=None):
    """``EventLists`` x ``EventReference`` of the same batch -> ``(acc, ct)`` GPU tensors: ``acc`` (S,C,4) int64 of (Ntp, Nfp,
    Nsys, Nref) and ``ct`` (S,C,C) int64 cross triggers indexed [reference class][estimated class], summed over the
    evaluated clips and ADDED into ``out = (acc, ct)`` when given (the accumulators of a validation pass).  The
    intersection criteria of psds_eval as include/bsed.h states them (``bsed_intersection_counts``; parity with psds_eval
    not pinned): an estimated event passes DTC when the reference events of its class cover at least ``dtc`` of it, is a
    false positive when it does not, and then cross-triggers every other class whose reference events cover at least
    ``cttc`` of it; a reference event is a true positive when the DTC-passing events of its class cover at least ``gtc``
    of it.  Two HIP launches, no host sync; no cap on the length of a list on either side."""
    who = "intersection_counts_gpu"
    if (events.B, events.C) != (reference.B, reference.C):
        raise BsedError(f"{who}: the events cover {events.B} clips x {events.C} classes, the reference "
                        f"{reference.B} x {reference.C}")
    S, B, C = events.S, events.B, events.C
    dev = events.offsets.device
    pair = f"an (({S}, {C}, 4), ({S}, {C}, {C})) pair of tensors"
    if out is None:
        out = (None, None)
    elif len(out) != 2:
        raise BsedError(f"{who}: out must be {pair}")
    out = (_accumulator(out[0], (S, C, 4), dev, who, pair), _accumulator(out[1], (S, C, C), dev, who, pair))
    for name, v in (("dtc", dtc), ("gtc", gtc), ("cttc", cttc)):
        if not 0.0 < float(v) <= 1.0:
            raise BsedError(f"{who}: {name} must lie in (0, 1], got {v!r}")
    if S * B * C == 0:
        return out
    if events.total > events.seconds.shape[0] or events.offsets.numel() != S * B * C + 1:
        raise BsedError(f"{who}: the event lists hold {events.seconds.shape[0]} rows and "
                        f"{events.offsets.numel()} offsets for {events.total} events in {S * B * C} groups")
    ref_off, ref_sec = reference.device()
    flags = torch.empty(events.seconds.shape[0], device=dev, dtype=torch.uint8)     # max(E, 1) bytes of scratch
    L.call("bsed_intersection_counts", L.ptr(events.offsets, torch.int32), L.ptr(events.seconds, torch.float64),
           L.ptr(ref_off, torch.int32), L.ptr(ref_sec, torch.float64), L.ptr(reference.device_evaluated(), torch.uint8),
           S, B, C, float(dtc), float(gtc), float(cttc), L.ptr(flags, torch.uint8), L.ptr(out[0], torch.int64),
           L.ptr(out[1], torch.int64), L.stream())
    return out


def intersection_f1(acc):
    """(..., C, 4) integer counts (Ntp, Nfp, Nsys, Nref) -> dict of float64 numpy arrays: ``class_f1`` (..., C) and ``macro``
    (...).  Per class F = 2 Ntp / (2 Ntp + Nfp + (Nref - Ntp)); F is NaN where Nref == 0 -- psds_eval's rule: a class
    without reference events is left out of the average even when it is predicted.  That DIFFERS from ``event_f1``, whose
    F is NaN only where the class neither occurs nor is predicted (and 0 where it is predicted but does not occur).
    ``macro`` is the mean over the classes whose F is not NaN, summed in class order (NaN if there is none)."""
    c = _host_counts(acc, 4, "intersection_f1 takes (..., C, 4) counts").astype(np.float64)
    ntp, nfp, nref = c[..., 0], c[..., 1], c[..., 3]
    class_f1 = np.divide(2.0 * ntp, 2.0 * ntp + nfp + (nref - ntp), out=np.full(ntp.shape, np.nan), where=nref > 0)
    return {"class_f1": class_f1, "macro": _macro_in_class_order(class_f1)}


def psds_rates(acc, ct, ref_duration, total_duration):
    """Counts -> dict of float64 rates, per hour where they are rates: ``tpr`` (S,C) = Ntp / Nref, NaN where Nref == 0;
    ``fpr`` (S,C) = Nfp / total_duration * 3600; ``ctr`` (S,C,C) = ct[s,k,j] / ref_duration[k] * 3600, NaN where
    ref_duration[k] == 0.  ``ref_duration`` (C): the summed length in seconds of every class's reference events over the
    evaluated clips (``EventReference.class_durations``); ``total_duration``: the summed duration of the evaluated clips."""
    a = _host_counts(acc, 4, "psds_rates takes (S, C, 4) counts").astype(np.float64)
    x = _host_counts(ct, a.shape[-2], "psds_rates takes an (S, C, C) cross-trigger matrix").astype(np.float64)
    dur = np.asarray(ref_duration, np.float64)
    if a.ndim != 3 or x.shape != a.shape[:2] + (a.shape[1],) or dur.shape != (a.shape[1],):
        raise BsedError(f"psds_rates: counts {a.shape}, cross triggers {x.shape} and durations {dur.shape} do not belong together")
    tpr = np.divide(a[..., 0], a[..., 3], out=np.full(a.shape[:2], np.nan), where=a[..., 3] > 0)
    fpr = a[..., 1] / float(total_duration) * 3600.0
    per_k = np.broadcast_to(dur[None, :, None], x.shape)
    ctr = np.divide(x, per_k, out=np.full(x.shape, np.nan), where=per_k != 0) * 3600.0
    return {"tpr": tpr, "fpr": fpr, "ctr": ctr}


class PsdsScore:
    """``PsdsResult.psds``'s return value: ``value``, and the curve it is the area under: ``efpr`` (the axis up to
    ``max_efpr``, per hour) and ``etpr`` (the effective true-positive rate held from each point to the next)"""

    def __init__(self, value, efpr, etpr, alpha_ct, alpha_st, max_efpr):
        self.value, self.efpr, self.etpr = float(value), efpr, etpr
        self.alpha_ct, self.alpha_st, self.max_efpr = alpha_ct, alpha_st, max_efpr

    def __repr__(self):
        return f"PsdsScore(value={self.value:.5f}, alpha_ct={self.alpha_ct}, alpha_st={self.alpha_st}, max_efpr={self.max_efpr})"


def psds_from_rates(tpr, efpr, alpha_st=0.0, max_efpr=100.0):
    """(S,C) true-positive rates and effective false-positive rates of S operating points -> ``(value, axis, curve)``.
    Per class the points are ordered by (efpr, tpr) and tpr replaced by its running maximum; on the union of all finite
    efpr values each class curve holds its previous value (a left-held step, 0 before the class's first point; a class
    whose tpr is NaN -- no reference event -- is NaN throughout); across classes ``nanmean - alpha_st * nanstd`` (ddof 0);
    ``max_efpr`` is inserted into the axis with the held value if absent; the area is ``sum(diff(x) * y[:-1])`` over
    ``x <= max_efpr``, divided by ``max_efpr``."""
    tpr, efpr = np.asarray(tpr, np.float64), np.asarray(efpr, np.float64)
    if tpr.ndim != 2 or tpr.shape != efpr.shape:
        raise BsedError(f"psds_from_rates takes (S, C) tpr and efpr, got {tpr.shape} and {efpr.shape}")
    if not max_efpr > 0:
        raise BsedError(f"psds_from_rates: max_efpr must be positive, got {max_efpr!r}")
    S, C = tpr.shape
    axis = np.unique(np.concatenate([efpr[np.isfinite(efpr)], [float(max_efpr)]]))
    axis = axis[axis <= max_efpr]
    curves = np.full((C, len(axis)), np.nan)
    for c in range(C):
        if np.isnan(tpr[:, c]).any():
            continue
        ok = np.isfinite(efpr[:, c])
        curves[c] = 0.0
        if not ok.any():
            continue
        x, y = efpr[ok, c], tpr[ok, c]
        order = np.lexsort((y, x))
        x, y = x[order], np.maximum.accumulate(y[order])
        at = np.searchsorted(x, axis, side="right") - 1         # the last point with efpr <= the axis value
        curves[c] = np.where(at >= 0, y[np.maximum(at, 0)], 0.0)
    live = ~np.isnan(curves).all(1)
    if not live.any():
        return float("nan"), axis, np.full(len(axis), np.nan)
    curve = curves[live].mean(0) - alpha_st * curves[live].std(0)
    return float(np.sum(np.diff(axis) * curve[:-1]) / max_efpr), axis, curve


class PsdsResult:
    """The intersection-based result of S operating points (thresholds): ``counts`` (S,C,4) int64 numpy (Ntp, Nfp, Nsys,
    Nref), ``ct`` (S,C,C) int64 cross triggers [reference class][estimated class], ``class_f1`` (S,C) / ``macro_f1`` (S)
    (``intersection_f1``), ``tpr`` / ``fpr`` (S,C) and ``ctr`` (S,C,C) (``psds_rates``), ``ref_duration`` (C),
    ``total_duration``, ``criteria`` = (dtc, gtc, cttc), ``labels``, ``thresholds``.  ``psds(alpha_ct, alpha_st, max_efpr)``
    is psds_eval's score as this project states it (include/bsed.h; parity with psds_eval not pinned)."""

    def __init__(self, counts, ct, ref_duration, total_duration, labels=None, thresholds=None, criteria=(0.5, 0.5, 0.3)):
        self.counts = _host_counts(counts, 4, "PsdsResult takes (S, C, 4) counts").astype(np.int64)
        self.ct = _host_counts(ct, self.counts.shape[-2], "PsdsResult takes an (S, C, C) cross-trigger matrix").astype(np.int64)
        self.ref_duration = np.asarray(ref_duration, np.float64)
        self.total_duration = float("nan") if total_duration is None else float(total_duration)
        self.labels = None if labels is None else list(labels)
        self.thresholds = None if thresholds is None else list(thresholds)
        self.criteria = tuple(criteria)
        f = intersection_f1(self.counts)
        self.class_f1, self.macro_f1 = f["class_f1"], f["macro"]
        r = psds_rates(self.counts, self.ct, self.ref_duration, self.total_duration)
        self.tpr, self.fpr, self.ctr = r["tpr"], r["fpr"], r["ctr"]

    def efpr(self, alpha_ct=0.0):
        """(S,C) effective false-positive rate: ``fpr[s,c] + alpha_ct * (mean over k != c of ctr[s,k,c])``, the mean over
        the classes k whose rate is not NaN, summed in class order; the term is left out when ``alpha_ct == 0`` and
        where no other class has a rate (one class, or no other class with reference events)"""
        if alpha_ct == 0:
            return self.fpr.copy()
        S, C = self.fpr.shape
        total, n = np.zeros((S, C)), np.zeros((S, C))
        for k in range(C):
            use = ~np.isnan(self.ctr[:, k, :])
            use[:, k] = False
            total, n = total + np.where(use, self.ctr[:, k, :], 0.0), n + use
        return self.fpr + np.where(n > 0, alpha_ct * (total / np.maximum(n, 1)), 0.0)

    def psds(self, alpha_ct=0, alpha_st=0, max_efpr=100):
        """-> ``PsdsScore`` with ``.value``, ``.efpr`` and ``.etpr`` (``psds_from_rates`` on ``tpr`` and ``efpr(alpha_ct)``)"""
        if not np.isfinite(self.total_duration) or self.total_duration <= 0:
            raise BsedError("PsdsResult.psds: the false-positive rates need the total duration of the evaluated audio")
        value, axis, curve = psds_from_rates(self.tpr, self.efpr(alpha_ct), alpha_st, max_efpr)
        return PsdsScore(value, axis, curve, alpha_ct, alpha_st, max_efpr)
