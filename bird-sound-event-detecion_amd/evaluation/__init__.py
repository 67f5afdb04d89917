"""Inference, event decoding and scoring -- host-side mirror of the reference's ``get_predictions`` and of what its
drivers do with the result.  Everything per frame runs on the GPU for the whole batch; only event lists and integer
counts travel to the host.  One module per subject, each importing only from those listed before it:

  _common       what every pass shares: eval-mode forward, loader batches, annotation files, the prediction frame, the
                count-then-write launches of a decoder, and the scorers' host helpers
  clips         ``get_predictions`` <- reference src/evaluation_measures.py:123-283: threshold + median filter
                (``binarize_median_gpu``, class-wise with ``learned_post``), contiguous regions and frames -> seconds
                (``decode_regions_gpu``), ground-truth and duration frames; ``post_process`` is the host restatement
  recording     ``detect_recording`` <- no counterpart in the reference, which only ever sees 10 s clips: ``window_plan`` ->
                ``gather_windows`` -> the clip path -> ``stitch_windows`` -> ``decode_long_gpu``
  events        ``EventLists`` of ALL thresholds from one pair of launches (``sweep_events_gpu``), ``EventReference``, the
                collar-based sed_eval counts (``event_counts_gpu``) and ``event_f1``
  intersection  psds_eval's criteria as include/bsed.h states them (parity not pinned): ``intersection_counts_gpu``,
                ``intersection_f1``, ``psds_rates``, ``psds_from_rates``, ``PsdsResult``
  tagging       the clip-level side <- src/evaluation_measures.py:346-446, src/audio_tagging_inference.py:289-316:
                ``tag_counts_gpu``, ``validate_weak``, ``get_f_measure_by_class``, ``pseudo_label``
  validation    ``validate`` <- the reference's per-epoch validation (src/main_baseline.py:1010-1032) over a threshold
                sweep, ``score_recording`` for a ``detect_recording`` result, and the DataFrame drop-ins ``compute_metrics``
                and ``compute_psds_from_operating_points``

sed_eval's segment-based metric lives beside the package, in ``bsed_amd.segment_metrics`` (``segment_counts_gpu``,
``SegmentResult``, ``compute_sed_eval_metrics``); ``validate`` and ``score_recording`` call it on request (``segment=``).
"""
from .._lib import BsedError
# the private helpers that tools/ and earlier tests import from here keep resolving; they are not part of __all__
from ._common import _eval_mode, _event_frame, _forward, _read_annotations  # noqa: F401
from .clips import (MEDIAN_WINDOW_S_CLASSWISE, binarize_median_classwise_gpu, binarize_median_gpu, classwise_median_windows,
                    decode_regions_gpu, get_predictions, post_process)
from .events import _event_table  # noqa: F401
from .events import MATCH_MAX_REF, EventLists, EventReference, event_counts_gpu, event_f1, sweep_events_gpu
from .intersection import PsdsResult, PsdsScore, intersection_counts_gpu, intersection_f1, psds_from_rates, psds_rates
from .recording import decode_long_gpu, detect_recording, gather_windows, stitch_windows, window_plan
from .tagging import (TAG_MASK_MAX_CLASSES, TaggingResult, TagThresholds, get_f_measure_by_class, pseudo_label,
                      pseudo_label_frame, tag_counts_gpu, tag_f1, tag_masks_gpu, validate_weak)
from .validation import (ValidationResult, compute_metrics, compute_psds_from_operating_points, recording_problem,
                         score_recording, validate)

__all__ = [
    "BsedError", "MEDIAN_WINDOW_S_CLASSWISE", "binarize_median_classwise_gpu", "binarize_median_gpu",
    "classwise_median_windows", "decode_regions_gpu", "get_predictions", "post_process",
    "decode_long_gpu", "detect_recording", "gather_windows", "stitch_windows", "window_plan",
    "MATCH_MAX_REF", "EventLists", "EventReference", "event_counts_gpu", "event_f1", "sweep_events_gpu",
    "PsdsResult", "PsdsScore", "intersection_counts_gpu", "intersection_f1", "psds_from_rates", "psds_rates",
    "TAG_MASK_MAX_CLASSES", "TaggingResult", "TagThresholds", "get_f_measure_by_class", "pseudo_label", "pseudo_label_frame",
    "tag_counts_gpu", "tag_f1", "tag_masks_gpu", "validate_weak", "ValidationResult", "compute_metrics",
    "compute_psds_from_operating_points", "recording_problem", "score_recording", "validate",
]
