"""Clip predictions: threshold + median filter, contiguous-region decode and ``get_predictions``, the mirror of the
reference's src/evaluation_measures.py:123-283."""
import os

import numpy as np
import torch

from .. import _lib as L
from ._common import (_EVENT_COLUMNS, _batches, _check_form, _count_then_write, _encoder_labels, _eval_mode, _event_frame,
                      _forward, _no_events, _read_annotations, _write_tsv)


def _seconds(events, scale, max_len_seconds):
    """``[label, onset frame, offset frame]`` rows of a decoder -> ``[label, onset_s, offset_s]`` clipped to the clip"""
    return [[lab, float(np.clip(on * scale, 0, max_len_seconds)), float(np.clip(off * scale, 0, max_len_seconds))]
            for lab, on, off in events]


def post_process(pred_strong, decoder, threshold=0.5, median_window=1, pooling_time_ratio=1, sr=32000,
                 hop_size=255, max_len_seconds=10.0):
    """Host restatement for ONE clip ((T', C) probabilities -> list of [event_label, onset_s, offset_s]); kept for
    callers that hand in a custom ``decoder`` function (the GPU decode needs the label list of a ManyHotEncoder)."""
    import scipy.ndimage
    binar = (np.asarray(pred_strong) > threshold).astype(np.float64)
    binar = scipy.ndimage.median_filter(binar, (median_window, 1))
    return _seconds(decoder(binar), pooling_time_ratio / (sr / hop_size), max_len_seconds)


def binarize_median_gpu(pred_strong, threshold=0.5, median_window=1):
    """(B,T',C) GPU probabilities -> (B,T',C) 0/1 mask: threshold + scipy-compatible median filter, one HIP kernel
    for the whole batch instead of a per-clip scipy call"""
    x = pred_strong.contiguous()
    B, T, C = x.shape
    out = torch.empty_like(x)
    L.call("bsed_binarize_median", L.ptr(x), L.ptr(out), B, T, C, threshold, median_window, L.stream())
    return out


def decode_regions_gpu(mask, scale, max_len_seconds):
    """(B,T',C) 0/1 GPU mask -> (clip (E,), class (E,), frames (E,2), seconds (E,2)) numpy arrays, ordered by clip,
    class, time: ManyHotEncoder.decode_strong for every clip of the batch plus the frames -> seconds conversion, in
    two HIP launches (count, write at the exclusive prefix of the counts)."""
    mask = mask.contiguous()
    B, T, C = mask.shape
    if B * C == 0 or T == 0:                            # an empty batch decodes to an empty event list
        return _no_events()
    _, E, outs = _count_then_write(
        B * C, mask.device, ("clip", "class", "frames", "seconds"),
        lambda counts: L.call("bsed_decode_count", L.ptr(mask), B, T, C, counts, L.stream()),
        lambda offsets, *ev: L.call("bsed_decode_write", L.ptr(mask), offsets, B, T, C, scale, max_len_seconds, *ev, L.stream()))
    return tuple(o[:E].cpu().numpy() for o in outs)


# reference src/data/config.py:62-63: cfg.median_window = [max(int(s * out_nb_frames_1s), 1) for s in median_window_s_classwise]
MEDIAN_WINDOW_S_CLASSWISE = [0.45, 0.45, 0.45, 0.45, 0.45, 2.7, 2.7, 2.7, 0.45, 2.7]


def classwise_median_windows(sr=32000, hop_size=255, pooling_time_ratio=4, seconds=MEDIAN_WINDOW_S_CLASSWISE):
    out_nb_frames_1s = sr / hop_size / pooling_time_ratio
    return [max(int(s * out_nb_frames_1s), 1) for s in seconds]


def _learned_windows(learned_post, classwise_median_window, sr, hop_size, pooling_time_ratio):
    """the ``classwise_median_window`` argument of a pass: with ``learned_post`` and no list given, the reference's
    ``cfg.median_window`` for this sr / hop / pooling"""
    if learned_post and classwise_median_window is None:
        return classwise_median_windows(sr, hop_size, pooling_time_ratio)
    return classwise_median_window


def binarize_median_classwise_gpu(pred_strong, threshold, windows):
    """``learned_post`` of the reference (src/evaluation_measures.py:192-197): class k gets its own median window
    ``windows[k]``; like the reference's ``np.hstack`` over ``range(len(cfg.median_window))``, classes beyond the list
    are dropped (no events).  One HIP launch per DISTINCT window, columns merged on the GPU."""
    B, T, C = pred_strong.shape
    out = torch.zeros_like(pred_strong)
    for w in sorted(set(windows[:C])):
        cols = torch.tensor([k for k, wk in enumerate(windows[:C]) if wk == w], device=pred_strong.device)
        out[:, :, cols] = binarize_median_gpu(pred_strong, threshold, w)[:, :, cols]
    return out


def _threshold_mask(pred_strong, threshold, median_window, learned_post, classwise_median_window):
    """the 0/1 mask of ONE threshold: class-wise windows with ``learned_post``, else one window for every class"""
    if learned_post:
        return binarize_median_classwise_gpu(pred_strong, threshold, list(classwise_median_window))
    return binarize_median_gpu(pred_strong, threshold, median_window)


def get_predictions(model, dataloader, decoder, pooling_time_ratio=1, thresholds=(0.5,), median_window=1,
                    save_predictions=None, del_model=False, learned_post=False, predictor=None, fpn=False,
                    saved_feature_dir=None, sr=32000, hop_size=255, max_len_seconds=10.0, classwise_median_window=None,
                    require_annotations=False):
    """Same call signature and return value as the reference: ``(predictions, groundtruth_df, duration_df)``.
    ``dataloader`` yields ``(((input, ema_input), target), paths)`` batches.  predictions: one DataFrame (or a list,
    one per threshold) with columns event_label / onset / offset / filename (seconds); groundtruth_df: the
    ``annotation/<name>.txt`` files of the clips concatenated with a ``filename`` column; duration_df: filename /
    duration (10, as the reference hard-codes it).
    learned_post: class-wise median windows (``classwise_median_window``, default the reference's ``cfg.median_window``
    list for this sr / hop / pooling).  predictor=None: ``model`` returns ``(strong, weak)`` itself and is called as
    ``model(x, inference=True)`` when ``fpn`` (reference :180-181; its ``seg_index`` form belongs to a model class that is
    not on the path).  Clips without an ``annotation/<name>.txt`` (unlabelled / pseudo-labelled sets) are left out of
    groundtruth_df -- None when no clip has one -- unless ``require_annotations`` (the reference's behaviour: it raises).
    Everything per frame runs on the GPU for the whole batch; only the event list (a few rows per clip) travels to the
    host, where the DataFrames are assembled without a per-clip Python loop.  Optional embedding dump
    ``<saved_feature_dir>/<i>.npy`` (what save_features.py is for)."""
    import pandas as pd
    _check_form("get_predictions", predictor, fpn)
    classwise_median_window = _learned_windows(learned_post, classwise_median_window, sr, hop_size, pooling_time_ratio)
    labels = _encoder_labels(decoder, "decode_strong")
    scale = pooling_time_ratio / (sr / hop_size)
    frames = {t: [] for t in thresholds}
    filename_list, annotation_folder_list = [], []
    with _eval_mode(model, predictor):
        for i, (x, _target, _paths, names, folders) in enumerate(_batches(dataloader, clips=True)):
            pred_strong, _, feature_out = _forward(model, predictor, fpn, x, features=True)
            if saved_feature_dir is not None and feature_out is not None:
                np.save(os.path.join(saved_feature_dir, f"{i}"), feature_out.cpu().numpy())
            for t in thresholds:
                mask = _threshold_mask(pred_strong, t, median_window, learned_post, classwise_median_window)
                if labels is not None:
                    ev_clip, ev_class, _, ev_sec = decode_regions_gpu(mask, scale, max_len_seconds)
                    frames[t].append(_event_frame(labels, ev_class, ev_sec, np.asarray(names, dtype=object)[ev_clip]))
                else:
                    # a caller-supplied decoder function can only run on the host, clip by clip
                    rows = [row + [names[j]] for j, m in enumerate(mask.cpu().numpy())
                            for row in _seconds(decoder(m), scale, max_len_seconds)]
                    frames[t].append(pd.DataFrame(rows, columns=_EVENT_COLUMNS))
            filename_list += names
            annotation_folder_list += folders
    dfs = [pd.concat(frames[t], ignore_index=True)[_EVENT_COLUMNS] if frames[t] else pd.DataFrame(columns=_EVENT_COLUMNS)
           for t in thresholds]

    # ground-truth and duration frames (reference :226-247): first occurrence of every file name, its annotation file
    # next to the features, duration 10
    duration_df = pd.DataFrame(list(dict.fromkeys(filename_list)), columns=["filename"])
    duration_df["duration"] = 10
    gts, n_found = _read_annotations(filename_list, annotation_folder_list, require_annotations)
    groundtruth_df = None
    if gts:
        groundtruth_df = pd.concat(gts, ignore_index=True)
    elif n_found:
        groundtruth_df = pd.DataFrame(columns=["onset", "offset", "event_label", "filename"])

    if save_predictions is not None:
        if isinstance(save_predictions, str):
            base, ext = os.path.splitext(save_predictions)
            outs = [save_predictions] if len(thresholds) == 1 else [os.path.join(base, f"{t:.3f}{ext}") for t in thresholds]
        else:
            assert len(save_predictions) == len(thresholds), \
                f"There should be a prediction file per threshold: {len(save_predictions)} vs {len(thresholds)}"
            outs = list(save_predictions)
        for df, path in zip(dfs, outs):
            _write_tsv(df, path, float_format="%.3f")
    predictions = dfs[0] if len(dfs) == 1 else dfs
    return predictions, groundtruth_df, duration_df
