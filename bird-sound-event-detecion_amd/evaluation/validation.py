"""Scoring passes.  ``validate`` is the reference's per-epoch validation (src/main_baseline.py:1010-1032:
``get_predictions`` -> ``compute_metrics`` -> sed_eval event-based F1, t_collar 0.2 s, 20 % of the length on the offset,
macro average) and its threshold sweep, with -- on request -- the clip-level counts of ``tagging`` and the intersection
counts of ``intersection`` from the same pass; ``score_recording`` applies the same counts to a ``detect_recording``
result; ``compute_metrics`` (src/evaluation_measures.py:518-526) and ``compute_psds_from_operating_points`` (:505-510)
are the drop-ins for DataFrames.  sed_eval's segment-based metric, the other half of the reference's
``compute_sed_eval_metrics`` (:318-325), is counted from the same event lists on request (``segment=``; the scorer itself
is ``bsed_amd.segment_metrics``, beside this package)."""
import numpy as np
import torch

from .._lib import BsedError
from ..segment_metrics import SegmentResult, _resolution, segment_counts_gpu
from ._common import _EVENT_COLUMNS, _batches, _check_form, _eval_mode, _forward, _required_labels
from .clips import _learned_windows
from .events import (MATCH_MAX_REF, EventLists, EventReference, _annotation_reference, _frame_lists, _grouped_lists, _sweep,
                     _sweep_thresholds, _sweep_windows, event_counts_gpu, event_f1)
from .intersection import PsdsResult, _criteria, intersection_counts_gpu, intersection_f1
from .tagging import TaggingResult, TagThresholds, _loader_targets, tag_counts_gpu


def _meta_names(groundtruth_df, meta_df):
    """the clips of a scoring call: the files of ``meta_df`` in order, else those of the ground truth -> (names, durations)"""
    if meta_df is not None and len(meta_df):
        names = list(dict.fromkeys(meta_df["filename"]))
        first = meta_df.drop_duplicates("filename").set_index("filename")["duration"]
        return names, np.asarray([float(first[n]) for n in names], np.float64)
    if groundtruth_df is None or len(groundtruth_df) == 0:
        raise BsedError("scoring needs the files of meta_df (filename / duration) or a ground truth")
    names = list(dict.fromkeys(groundtruth_df["filename"]))
    return names, np.full(len(names), np.nan)


def compute_psds_from_operating_points(list_predictions, groundtruth_df, meta_df, labels, dtc_threshold=0.5,
                                       gtc_threshold=0.5, cttc_threshold=0.3):
    """The reference's call (src/evaluation_measures.py:505-510) without psds_eval: one prediction frame per operating
    point + ground truth + ``meta_df`` (filename / duration) -> ``PsdsResult``, whose ``.psds(alpha_ct, alpha_st,
    max_efpr).value`` is what ``psds_score`` prints.  ``labels``: the class list (psds_eval takes it from the ground
    truth).  Files of ``meta_df`` without a row in the ground truth are not evaluated and do not count in the duration."""
    dfs = list(list_predictions) if isinstance(list_predictions, (list, tuple)) else [list_predictions]
    names, durations = _meta_names(groundtruth_df, meta_df)
    reference = EventReference.from_frame(groundtruth_df, labels, names)
    events = _frame_lists(dfs, list(labels), names, "compute_psds_from_operating_points")
    criteria = (float(dtc_threshold), float(gtc_threshold), float(cttc_threshold))
    acc, ct = intersection_counts_gpu(events, reference, *criteria)
    total = float(np.cumsum(durations[reference.evaluated])[-1]) if reference.evaluated.any() else 0.0
    return PsdsResult(acc, ct, reference.class_durations(), total, labels, None, criteria)


def compute_metrics(predictions, gtruth_df, meta_df, labels):
    """The reference's per-epoch scoring (src/evaluation_measures.py:518-526) on DataFrames -> ``(ct_matrix, macro_f1_event,
    psds_macro_f1)``: the (C,C) int64 cross-trigger matrix [reference class][estimated class] at (dtc, gtc, cttc) =
    (0.5, 0.5, 0.3) (psds_eval's has one more row and column, for its "world" label), the collar-based macro event F1
    (``event_counts_gpu`` / ``event_f1``: t_collar 0.2 s, 20 % of the length) and the intersection-based macro F1
    (``intersection_f1``), both counted on the GPU."""
    names, _ = _meta_names(gtruth_df, meta_df)
    reference = EventReference.from_frame(gtruth_df, labels, names)
    events = _frame_lists([predictions], list(labels), names, "compute_metrics")
    macro_f1_event = float(event_f1(event_counts_gpu(events, reference))["macro"][0])
    acc, ct = intersection_counts_gpu(events, reference)
    return ct[0].cpu().numpy(), macro_f1_event, float(intersection_f1(acc)["macro"][0])


class ValidationResult:
    """``validate``'s return value: ``thresholds`` (list), ``counts`` (S,C,3) int64 numpy (Ntp, Nsys, Nref), ``class_f1``
    (S,C), ``macro_f1`` / ``micro_f1`` (S), ``best_index`` / ``best_threshold`` (highest macro F, ties to the lowest
    threshold; NaN counts as lowest), ``labels``, and -- on request -- ``predictions`` (one DataFrame per threshold) and
    ``groundtruth_df``; ``tagging``: the ``TaggingResult`` of the same pass when ``validate`` was given
    ``tagging_thresholds``, else None; ``intersection``: the ``PsdsResult`` of the same pass when ``validate`` was given
    ``intersection``, else None; ``segment``: the ``SegmentResult`` of the same pass when ``validate`` was given ``segment``,
    else None."""

    def __init__(self, thresholds, counts, labels, predictions=None, groundtruth_df=None, tagging=None, intersection=None,
                 segment=None):
        self.thresholds, self.counts, self.labels = list(thresholds), counts, list(labels)
        f = event_f1(counts)
        self.class_f1, self.macro_f1, self.micro_f1 = f["class_f1"], f["macro"], f["micro"]
        key = np.where(np.isnan(self.macro_f1), -np.inf, self.macro_f1)
        best = np.nonzero(key == key.max())[0]
        self.best_index = int(min(best, key=lambda i: (self.thresholds[i], i)))
        self.best_threshold = self.thresholds[self.best_index]
        self.best_macro_f1 = float(self.macro_f1[self.best_index])
        self.predictions, self.groundtruth_df = predictions, groundtruth_df
        self.tagging = tagging
        self.intersection = intersection
        self.segment = segment


def validate(model, dataloader, decoder, predictor=None, fpn=False, thresholds=(0.5,), median_window=1, learned_post=False,
             t_collar=0.2, percentage_of_length=0.2, pooling_time_ratio=1, sr=32000, hop_size=255, max_len_seconds=10.0,
             classwise_median_window=None, return_predictions=False, require_annotations=False, ignore_unknown=False,
             tagging_thresholds=None, intersection=None, segment=None):
    """One validation pass, scored on the GPU: the eval-mode forward of ``get_predictions`` (same ``dataloader``, ``decoder``,
    ``predictor`` / ``fpn`` forms and the same ``annotation/<name>.txt`` files), every batch swept over ALL ``thresholds``
    (``sweep_events_gpu``: one host sync per batch) and matched against its reference (``event_counts_gpu``), the counts
    accumulated on the device and read once at the end.  Returns a ``ValidationResult``: the counts, per-class / macro /
    micro event F1 per threshold and the best threshold by macro F1 -- the number the reference keeps ``baseline_best``
    by.  The prediction frames (as ``get_predictions`` returns them per threshold) and the ground-truth frame are built
    only with ``return_predictions``.  A clip name may occur once per pass.  Training flags are restored on exit.
    ``tagging_thresholds`` (opt-in): the weak output of the same forward is scored against the loader's own targets over
    these thresholds (``tag_counts_gpu``, one more launch per batch) and the ``TaggingResult`` hangs on ``.tagging``; with
    the default None the pass launches and returns what it did without the argument.
    ``intersection`` (opt-in): True, or a ``(dtc, gtc, cttc)`` tuple (True = (0.5, 0.5, 0.3)): the same event lists are also
    scored by the intersection criteria (``intersection_counts_gpu``, one more call per batch, accumulated on the device
    and read once at the end) and the ``PsdsResult`` -- counts, cross-trigger matrix, class and macro intersection F1 per
    threshold, ``.psds(...)`` over the thresholds as operating points -- hangs on ``.intersection``; every evaluated clip
    counts ``max_len_seconds`` in the total duration.  With None the pass launches and returns what it did without it.
    ``segment`` (opt-in): True (time resolution 1.0 s, the reference's value) or a positive resolution in seconds: the same
    event lists are also scored by sed_eval's segment-based metric as the reference calls it, with no evaluated length
    (``segment_counts_gpu``, one more call per batch, accumulated on the device and read once at the end) and the
    ``SegmentResult`` hangs on ``.segment``.  With None the pass launches and returns what it did without it."""
    import pandas as pd
    _check_form("validate", predictor, fpn)
    criteria = _criteria(intersection, "validate")
    resolution, seg_acc = _resolution(segment, "validate"), None
    isect_acc, ref_duration, n_evaluated = None, None, 0
    labels = _required_labels(decoder, "decode_strong", "validate", "decodes and scores")
    thresholds = [float(t) for t in thresholds]
    classwise_median_window = _learned_windows(learned_post, classwise_median_window, sr, hop_size, pooling_time_ratio)
    scale = pooling_time_ratio / (sr / hop_size)
    thr, win, acc = _sweep_thresholds(thresholds), None, None
    tag_thr, tag_acc = (None if tagging_thresholds is None else TagThresholds(tagging_thresholds)), None
    frames, gts, seen = [[] for _ in thresholds], [], set()
    with _eval_mode(model, predictor):
        for x, target, _paths, names, folders in _batches(dataloader, clips=True):
            if seen & set(names):
                raise BsedError(f"validate: clip(s) {sorted(seen & set(names))[:3]} occur in more than one batch")
            seen |= set(names)
            pred_strong, pred_weak, _ = _forward(model, predictor, fpn, x, weak=tag_thr is not None)
            if tag_thr is not None:
                tag_acc = tag_counts_gpu(pred_weak, _loader_targets(target, "validate(tagging_thresholds=...)"), tag_thr,
                                         out=tag_acc)
            pred_strong = pred_strong.contiguous()
            C = pred_strong.shape[2]
            if C > len(labels):
                raise BsedError(f"validate: the model returned {C} classes, the decoder has {len(labels)} labels")
            if win is None:
                win = _sweep_windows(median_window, classwise_median_window if learned_post else None, C)
                acc = torch.zeros((len(thresholds), C, 3), device=pred_strong.device, dtype=torch.int64)
            events = _sweep(pred_strong, thr, win, scale, float(max_len_seconds))
            reference, dfs = _annotation_reference(names, folders, labels[:C], ignore_unknown, require_annotations)
            event_counts_gpu(events, reference, t_collar, percentage_of_length, out=acc)
            if criteria is not None:
                isect_acc = intersection_counts_gpu(events, reference, *criteria, out=isect_acc)
                durations = reference.class_durations()
                ref_duration = durations if ref_duration is None else ref_duration + durations
                n_evaluated += int(reference.evaluated.sum())
            if resolution is not None:
                seg_acc = segment_counts_gpu(events, reference, resolution, out=seg_acc,
                                             expected_seconds=max(float(max_len_seconds), resolution))
            if return_predictions:
                gts += dfs
                for s, df in enumerate(events.frames(labels, names)):
                    frames[s].append(df)
    if acc is None:
        raise BsedError("validate: the dataloader yielded no batch")
    predictions = groundtruth_df = None
    if return_predictions:
        predictions = [pd.concat(f, ignore_index=True)[_EVENT_COLUMNS] for f in frames]
        groundtruth_df = pd.concat(gts, ignore_index=True) if gts else None
    tagging = None if tag_thr is None else TaggingResult(tag_thr.host, tag_acc.cpu().numpy(), labels[:tag_acc.shape[1]])
    isect = None
    if criteria is not None:
        isect = PsdsResult(isect_acc[0], isect_acc[1], ref_duration, n_evaluated * float(max_len_seconds),
                           labels[:acc.shape[1]], thresholds, criteria)
    seg = None if resolution is None else SegmentResult(*seg_acc, resolution, labels[:acc.shape[1]], thresholds)
    return ValidationResult(thresholds, acc.cpu().numpy(), labels[:acc.shape[1]], predictions, groundtruth_df, tagging, isect,
                            seg)


_SEGMENT_SLACK = 1e-6       # seconds; far above the rounding of second-valued float64 differences, far below any collar


def recording_problem(events_df, groundtruth_df, labels, t_collar=0.2, ignore_unknown=False):
    """Host preparation of ``score_recording`` -> ``(counts (S,B',C), est seconds, EventReference)``.  One recording has one
    long list per class, so the time line of every class is cut into independent pieces that play the part of clips: a
    hit needs the onsets within ``t_collar``, so where two neighbouring reference onsets of a class lie more than
    ``2 * t_collar`` (+ 1 us) apart no estimated event can hit on both sides, and the maximum matching is the sum over
    the pieces.  An estimated event goes to the piece whose onsets it can reach (to the nearest earlier one if none)."""
    labels = list(labels)
    C = len(labels)
    dfs = list(events_df) if isinstance(events_df, (list, tuple)) else [events_df]
    gap = 2.0 * float(t_collar) + _SEGMENT_SLACK
    starts = []                                         # per class: first onset of every piece

    def reference_pieces(k, on):
        piece = np.zeros(len(k), np.int64)              # piece index of every reference event inside its class
        for c in range(C):
            idx = np.nonzero(k == c)[0]
            idx = idx[np.argsort(on[idx], kind="stable")]
            new = np.concatenate([[True], np.diff(on[idx]) > gap]) if len(idx) else np.zeros(0, bool)
            piece[idx] = np.cumsum(new) - 1
            starts.append(on[idx][new])
        return piece, max([1] + [len(s) for s in starts])

    def estimated_pieces(k, on):
        piece = np.zeros(len(k), np.int64)
        for c in range(C):
            idx = np.nonzero(k == c)[0]
            if len(idx) and len(starts[c]):
                piece[idx] = np.maximum(np.searchsorted(starts[c] - float(t_collar) - _SEGMENT_SLACK / 2, on[idx], "right") - 1, 0)
        return piece, Bp

    def lists(df, what, pieces):                        # both sides sorted by (piece, class, onset, offset)
        return _grouped_lists(df, labels, None, "sorted", ignore_unknown=ignore_unknown and what == "reference", pieces=pieces,
                              unknown=lambda label, _b: f"score_recording: {what} event label {label!r} is not in the label list")

    ref_counts, ref_seconds, _ = lists(groundtruth_df, "reference", reference_pieces)
    Bp = len(ref_counts)
    reference = EventReference(ref_counts, ref_seconds, [f"piece {i}" for i in range(Bp)], labels)
    if ref_counts.max(initial=0) > MATCH_MAX_REF:
        b, c = np.unravel_index(int(np.argmax(ref_counts)), ref_counts.shape)
        raise BsedError(f"score_recording: {int(ref_counts[b, c])} reference events of class {labels[c]!r} from "
                        f"{starts[c][b]:.3f} s on follow each other within {gap:.3f} s; the matcher takes at most "
                        f"{MATCH_MAX_REF} per such run")
    counts, secs = np.zeros((len(dfs), Bp, C), np.int64), [np.zeros((0, 2))]
    for s, df in enumerate(dfs):
        counts[s], sec, _ = lists(df, "estimated", estimated_pieces)
        secs.append(sec)
    return counts, np.concatenate(secs), reference


def score_recording(events_df, groundtruth_df, labels, t_collar=0.2, percentage_of_length=0.2, ignore_unknown=False,
                    intersection=None, duration=None, segment=None):
    """The event counts of ``validate`` for ONE recording: ``events_df`` is what ``detect_recording`` returns (a DataFrame,
    or a list of them, one per threshold), ``groundtruth_df`` has onset / offset / event_label rows in seconds of the
    recording (rows with NaN are dropped).  Returns the (S,C,3) int64 numpy counts (Ntp, Nsys, Nref); ``event_f1`` turns
    them into F1.  The match kernel works on lists of at most 64 reference events, so each class's time line is first
    cut where two neighbouring reference onsets lie more than ``2 * t_collar`` apart (``recording_problem``); the cap that
    remains: at most 64 reference events of one class in a run whose neighbouring onsets all lie within ``2 * t_collar``.
    The estimated lists have no cap.
    ``intersection`` (opt-in, as for ``validate``): True or a ``(dtc, gtc, cttc)`` tuple returns ``(counts, PsdsResult)``
    instead: the recording scored as ONE clip by the intersection criteria (``intersection_counts_gpu``; no pieces and no
    cap: nothing is matched), each estimated list in the order of its frame, the reference sorted by onset.  ``duration``:
    the recording's length in seconds, which only ``PsdsResult.psds`` and the false-positive rates need.
    ``segment`` (opt-in, as for ``validate``): True or a positive time resolution in seconds adds a ``SegmentResult``: the
    recording scored as ONE clip by sed_eval's segment-based metric (``segment_counts_gpu``; no pieces and no cap), with
    ``duration``, when given, as the evaluated length (else the recording ends with its last event of either side).
    The return value by what was asked for:
      neither                       ``counts``
      ``intersection``              ``(counts, PsdsResult)``
      ``segment``                   ``(counts, SegmentResult)``
      ``intersection``, ``segment``  ``(counts, PsdsResult, SegmentResult)``"""
    counts, seconds, reference = recording_problem(events_df, groundtruth_df, labels, t_collar, ignore_unknown)
    events = EventLists.from_host(counts, seconds)
    event_counts = event_counts_gpu(events, reference, t_collar, percentage_of_length).cpu().numpy()
    criteria = _criteria(intersection, "score_recording")
    resolution = _resolution(segment, "score_recording")
    if criteria is None and resolution is None:
        return event_counts
    labels = list(labels)
    dfs = [df.assign(filename="recording") for df in (events_df if isinstance(events_df, (list, tuple)) else [events_df])]
    gt = None if groundtruth_df is None or len(groundtruth_df) == 0 else groundtruth_df.assign(filename="recording")
    whole = EventReference.from_frame(gt, labels, ["recording"], ignore_unknown)
    whole.evaluated[:] = True                           # a recording without a reference event is still scored
    lists, out = _frame_lists(dfs, labels, ["recording"], "score_recording"), (event_counts,)
    if criteria is not None:
        acc, ct = intersection_counts_gpu(lists, whole, *criteria)
        out += (PsdsResult(acc, ct, whole.class_durations(), duration, labels, None, criteria),)
    if resolution is not None:
        last = max(resolution, float(whole.seconds.max(initial=0.0)))       # sizes the launch when no duration is given
        out += (SegmentResult(*segment_counts_gpu(lists, whole, resolution, duration, expected_seconds=last), resolution,
                              labels),)
    return out
