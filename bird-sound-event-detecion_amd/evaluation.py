"""Inference / event decoding -- host-side mirror of the reference's ``get_predictions``.

  get_predictions   <- reference src/evaluation_measures.py:123-283: eval-mode forward, threshold, (median_window, 1)
                       median filter, ``decoder`` (ManyHotEncoder.decode_strong: contiguous regions), frames -> seconds
                       with ``pooling_time_ratio / (sr / hop)`` clipped to [0, max_len_seconds]; ground-truth frame
                       from ``annotation/<name>.txt`` next to the features, duration frame (10 s per clip); optional
                       embedding dump ``<saved_feature_dir>/<i>.npy`` (what save_features.py is for).
                       Returns ``(predictions, groundtruth_df, duration_df)`` like the reference (:283).
Everything per frame runs on the GPU for the whole batch: forward (HIP), threshold + median filter
(``bsed_binarize_median``), contiguous-region decode and the seconds conversion (``bsed_decode_count`` /
``bsed_decode_write``).  Only the event list (a few rows per clip) travels to the host, where the DataFrames are
assembled without a per-clip Python loop.  The collar-based event F1 that picks the best checkpoint is computed here too
(``validate`` below), and so are -- on request -- the intersection-based counts behind psds_eval's macro F1, its
cross-trigger matrix and PSDS (``intersection_counts_gpu``; rules as stated in include/bsed.h, parity with psds_eval not
pinned); the segment-based metric stays external.

  detect_recording  <- no counterpart in the reference, which cuts recordings into 10 s clips offline
                       (src/data/preprocess.py:176-229) and only ever sees clips: one whole recording -> overlapping
                       clip-sized windows on the recording's frame grid (``window_plan``, ``bsed_gather_windows``) -> the clip
                       path above -> one (T_total, C) time line (``stitch_windows``) -> threshold / median / contiguous
                       regions decoded in parallel over time (``decode_long_gpu``) -> events in seconds of the recording.

  validate          <- the reference's per-epoch validation (src/main_baseline.py:1010-1032: ``get_predictions`` ->
                       ``compute_metrics`` -> sed_eval event-based F1, t_collar 0.2 s, 20 % of the length on the offset,
                       macro average) and its threshold sweep: the event lists of ALL thresholds from one pair of launches
                       (``sweep_events_gpu``), Ntp / Nsys / Nref per (threshold, class) counted on the GPU with sed_eval's
                       optimal matching (``event_counts_gpu``), F1 from the integer counts on the host (``event_f1``).
                       ``score_recording`` applies the same counts to a ``detect_recording`` result.
                       ``intersection=True`` adds the second number of the reference's ``compute_metrics``
                       (src/evaluation_measures.py:518-526: psds_eval's intersection-based macro F1 with a cross-trigger
                       matrix) and what its inference drivers make of the sweep (:287-316, :505-510: PSDS at (0, 0, 100),
                       (1, 0, 100), (0, 1, 100)): DTC / GTC / CTTC counted on the GPU from the same event lists
                       (``intersection_counts_gpu``, two more launches per batch), F1 / rates / PSDS from the integer
                       counts on the host (``intersection_f1``, ``psds_rates``, ``PsdsResult``); ``compute_metrics`` and
                       ``compute_psds_from_operating_points`` are the drop-ins for DataFrames.

  validate_weak / get_f_measure_by_class / pseudo_label
                    <- the clip-level side: the reference's per-class weak F1 (src/evaluation_measures.py:346-446, the
                       number ``baseline_best`` is kept by in src/pseudo_labeling_main.py:990-1035) with the tp / fp / fn /
                       tn of a whole threshold sweep counted on the GPU (``tag_counts_gpu``, one launch per batch, read
                       once per pass), and the pseudo weak labels of an unlabelled pool
                       (src/audio_tagging_inference.py:289-316) as one bit mask per clip (``bsed_tag_masks``), written
                       as the ``filename<TAB>event_labels`` TSV that ``data.PseudoWeakDataset`` reads.
"""
import math
import os
from contextlib import contextmanager as _contextmanager
from fractions import Fraction

import numpy as np
import torch

from . import _lib as L
from ._lib import BsedError


_EVENT_COLUMNS = ["event_label", "onset", "offset", "filename"]


@_contextmanager
def _eval_mode(model, predictor=None):
    """``model`` and ``predictor`` (may be None) in eval mode for the body; their training flags come back on exit,
    also when the body raises"""
    was_training = (model.training, predictor.training if predictor is not None else False)
    model.eval()
    if predictor is not None:
        predictor.eval()
    try:
        yield
    finally:
        model.train(was_training[0])
        if predictor is not None:
            predictor.train(was_training[1])


def _check_form(who, predictor, fpn, trained=False):
    if predictor is None and not fpn and not trained:
        raise NotImplementedError(f"{who}: predictor=None without fpn=True is the reference's seg_index call of a model "
                                  "class outside the hot path; pass predictor=..., a self-contained model with fpn=True "
                                  "or, to the clip-level passes, trained=True")


def _forward(model, predictor, fpn, x, trained=False, weak=False, features=False):
    """One batch under no_grad in the reference's call forms (src/evaluation_measures.py:163-181, 373-385) ->
    ``(strong, weak, features)``.  ``weak`` and ``features`` (the encoder's second output, what ``saved_feature_dir``
    dumps) are taken from what the modules return only when asked for and are None otherwise; ``trained=True`` is the
    tagger's ``pred_weak = torch_model(batch_x)``: weak only, the weak part of a ``(strong, weak)`` return."""
    with torch.no_grad():
        if trained:
            out = model(x)
            return None, (out[1] if isinstance(out, (tuple, list)) else out), None
        if predictor is not None:
            encoded = model(x)
            out = predictor(encoded[0], inference=fpn)
        else:
            encoded, out = None, model(x, inference=True)
        return out[0], (out[1] if weak else None), (encoded[1] if features and encoded is not None else None)


def _batches(dataloader, clips=False):
    """the loader passes' unpack of ``(((input, ema_input), target), paths)`` batches -> ``(float32 GPU input, target,
    paths, names, folders)``; with ``clips`` the clip names and their ``annotation/`` folders next to the features
    (``<root>/wav/<name>.npy`` -> ``<name>``, ``<root>/annotation``), else None"""
    for ((input_data, _ema), target), paths in dataloader:
        names = folders = None
        if clips:
            names = [os.path.splitext(os.path.basename(p))[0] for p in paths]
            folders = [os.path.join(os.path.dirname(os.path.dirname(p)), "annotation") for p in paths]
        yield torch.as_tensor(input_data).float().cuda(), target, paths, names, folders


def _encoder_labels(decoder, method_name):
    """label list of the ManyHotEncoder whose bound ``method_name`` (``decode_strong`` / ``decode_weak``) was passed as
    ``decoder`` (the reference's call sites pass ``many_hot_encoder.decode_strong``, src/main_baseline.py:1010-1032, and
    ``.decode_weak``, src/audio_tagging_inference.py:287), or None for any other callable"""
    owner = getattr(decoder, "__self__", None)
    if owner is not None and getattr(decoder, "__name__", "") == method_name and hasattr(owner, "labels"):
        return list(owner.labels)
    return None


def _read_annotations(names, folders, require_annotations=False):
    """the ``annotation/<name>.txt`` files of these clips (first occurrence of a name), each with a ``filename`` column
    -> ``(list of the non-empty DataFrames, number of files found)``; a missing file is skipped (an unlabelled clip:
    predictions only) or, with ``require_annotations``, raises as the reference does"""
    import pandas as pd
    seen, out, n_found = {}, [], 0
    for name, folder in zip(names, folders):
        seen.setdefault(name, folder)
    for name, folder in seen.items():
        path = os.path.join(folder, name + ".txt")
        if not os.path.exists(path):
            if require_annotations:
                raise FileNotFoundError(f"annotation file {path} is missing (the reference reads annotation/<name>.txt next to "
                                        "wav/<name>.npy)")
            continue
        n_found += 1
        df = pd.read_csv(path, sep="\t")
        df["filename"] = name
        if len(df):
            out.append(df)
    return out, n_found


def _event_frame(labels, ev_class, seconds, filenames):
    """the prediction frame of every route: event_label (object) / onset / offset (float64) / filename (object), one row
    per event in the order given; ``filenames``: an object array, one entry per event"""
    import pandas as pd
    return pd.DataFrame({"event_label": np.asarray(labels, dtype=object)[ev_class], "onset": seconds[:, 0],
                         "offset": seconds[:, 1], "filename": filenames}, columns=_EVENT_COLUMNS)


_EVENT_OUTPUTS = {"clip": ((), torch.int32), "class": ((), torch.int32), "frames": ((2,), torch.int32),
                  "seconds": ((2,), torch.float64)}


def _no_events():
    return (np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros((0, 2), np.int32), np.zeros((0, 2), np.float64))


def _count_then_write(n, device, outputs, count, write):
    """The two launches of every decoder: ``count(counts)`` fills the ``n`` int32 list lengths, their prefix sum gives the
    place of every list and the total ``E`` -- read here, the one host sync of a decode --, the ``outputs`` (names of
    ``_EVENT_OUTPUTS``) are allocated with ``max(E, 1)`` rows and ``write(offsets, *outputs)`` fills them if there is an
    event.  The callbacks get device pointers.  -> ``(offsets (n + 1) int32: exclusive prefix, total last; E; tensors)``"""
    offsets = torch.zeros(n + 1, device=device, dtype=torch.int32)
    counts = torch.empty(n, device=device, dtype=torch.int32)
    count(L.ptr(counts, torch.int32))
    torch.cumsum(counts, 0, dtype=torch.int32, out=offsets[1:])
    E = int(offsets[-1])
    outs = [torch.empty((max(E, 1), *_EVENT_OUTPUTS[k][0]), device=device, dtype=_EVENT_OUTPUTS[k][1]) for k in outputs]
    if E:
        write(L.ptr(offsets, torch.int32), *(L.ptr(o, _EVENT_OUTPUTS[k][1]) for k, o in zip(outputs, outs)))
    return offsets, E, outs


def post_process(pred_strong, decoder, threshold=0.5, median_window=1, pooling_time_ratio=1, sr=32000,
                 hop_size=255, max_len_seconds=10.0):
    """Host restatement for ONE clip ((T', C) probabilities -> list of [event_label, onset_s, offset_s]); kept for
    callers that hand in a custom ``decoder`` function (the GPU decode needs the label list of a ManyHotEncoder)."""
    import scipy.ndimage
    binar = (np.asarray(pred_strong) > threshold).astype(np.float64)
    binar = scipy.ndimage.median_filter(binar, (median_window, 1))
    scale = pooling_time_ratio / (sr / hop_size)
    return [[lab, float(np.clip(on * scale, 0, max_len_seconds)), float(np.clip(off * scale, 0, max_len_seconds))]
            for lab, on, off in decoder(binar)]


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
    groundtruth_df -- None when no clip has one -- unless ``require_annotations`` (the reference's behaviour: it raises)."""
    import pandas as pd
    _check_form("get_predictions", predictor, fpn)
    if learned_post and classwise_median_window is None:
        classwise_median_window = classwise_median_windows(sr, hop_size, pooling_time_ratio)
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
                mask = (binarize_median_classwise_gpu(pred_strong, t, list(classwise_median_window)) if learned_post
                        else binarize_median_gpu(pred_strong, t, median_window))
                if labels is not None:
                    ev_clip, ev_class, _, ev_sec = decode_regions_gpu(mask, scale, max_len_seconds)
                    frames[t].append(_event_frame(labels, ev_class, ev_sec, np.asarray(names, dtype=object)[ev_clip]))
                else:
                    # a caller-supplied decoder function can only run on the host, clip by clip
                    rows = []
                    for j, m in enumerate(mask.cpu().numpy()):
                        for lab, on, off in decoder(m):
                            rows.append({"event_label": lab, "onset": float(np.clip(on * scale, 0, max_len_seconds)),
                                         "offset": float(np.clip(off * scale, 0, max_len_seconds)), "filename": names[j]})
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
            if len(thresholds) == 1:
                outs = [save_predictions]
            else:
                base, ext = os.path.splitext(save_predictions)
                outs = [os.path.join(base, f"{t:.3f}{ext}") for t in thresholds]
        else:
            assert len(save_predictions) == len(thresholds), \
                f"There should be a prediction file per threshold: {len(save_predictions)} vs {len(thresholds)}"
            outs = list(save_predictions)
        for df, path in zip(dfs, outs):
            if os.path.dirname(path):
                os.makedirs(os.path.dirname(path), exist_ok=True)
            df.to_csv(path, index=False, sep="\t", float_format="%.3f")
    predictions = dfs[0] if len(dfs) == 1 else dfs
    return predictions, groundtruth_df, duration_df


# ---------------------------------------------------------------------------------------------------------------------
# Recording-level detection
# ---------------------------------------------------------------------------------------------------------------------
def window_plan(n_samples, sr=32000, hop_size=255, pooling_time_ratio=4, max_len_seconds=10.0, hop_frames=None):
    """Window starts for a recording of ``n_samples`` -> ``(starts, Tp, T_total)``: ``starts`` int32 ascending, in OUTPUT
    FRAMES (one output frame = hop_size * pooling_time_ratio samples, 1020 at the reference configuration), ``Tp`` output
    frames per window, ``T_total = starts[-1] + Tp`` output frames of the recording.  Pure host arithmetic.

    A window that starts at sample ``1020 * s`` has its centred STFT frames, and so its pooled frames, exactly on the
    recording's frame grid: local output frame j of the window is frame s + j of the recording.  Windows have the clip
    length the model was trained on (``win = int(max_len_seconds * sr)`` samples, ``Tp = ceil(win / hop_size) //
    pooling_time_ratio``: 313 at 32 kHz, 216 at 22.05 kHz) and start every ``hop_frames`` (default ``Tp // 2``) while they
    fit; the LAST window is aligned to the end of the recording (start ``(n_samples - win) // 1020``, added only if it
    lies behind the last regular start), so no window holds padding and at most 1019 samples at the very end stay
    uncovered.  A recording shorter than one window is one window at 0, padded by the clip path.

    The reference's own cut, ``librosa.util.frame(audio, 320000, 320000)`` (src/data/preprocess.py:176-229), is NOT
    reproduced: 320000 / 1020 is not an integer, so its clips are off the frame grid, and it drops the tail.
    ``hop_frames = Tp`` is the closest setting (windows of 10 s every 9.977 s)."""
    n_samples, frame = int(n_samples), int(hop_size) * int(pooling_time_ratio)
    win = int(max_len_seconds * sr)
    Tp = math.ceil(win / hop_size) // pooling_time_ratio
    if n_samples < 1 or frame < 1 or Tp < 1:
        raise BsedError(f"window_plan: bad geometry (n_samples={n_samples}, frame={frame} samples, Tp={Tp})")
    hop_frames = Tp // 2 if hop_frames is None else int(hop_frames)
    if not 1 <= hop_frames <= Tp:
        raise BsedError(f"window_plan: hop_frames must be in 1..Tp={Tp}, got {hop_frames} (a larger hop leaves frames "
                        "that no window covers)")
    if n_samples <= win:
        return np.zeros(1, np.int32), Tp, Tp
    n_regular = (n_samples - win) // (hop_frames * frame) + 1           # starts s with 1020 s + win <= n_samples
    starts = [k * hop_frames for k in range(n_regular)]
    last = (n_samples - win) // frame
    if last > starts[-1]:
        starts.append(last)
    return np.asarray(starts, np.int32), Tp, starts[-1] + Tp


_WEIGHTINGS = {"uniform": "BSED_STITCH_UNIFORM", "triangular": "BSED_STITCH_TRIANGULAR"}


def _stitch_geometry(starts, Tp):
    """host check of the layout ``bsed_stitch_windows`` is built for -> hop_frames"""
    s = np.asarray(starts.cpu() if isinstance(starts, torch.Tensor) else starts).astype(np.int64).ravel()
    W = len(s)
    if W == 0 or s[0] != 0:
        raise BsedError("stitch_windows: starts must begin at frame 0")
    if W == 1:
        return s, Tp
    hop = int(s[1] - s[0])
    if not 1 <= hop <= Tp:
        raise BsedError(f"stitch_windows: windows must start 1..Tp={Tp} frames apart, got {hop}")
    if not np.array_equal(s[:-1], hop * np.arange(W - 1)) or not (W - 2) * hop < s[-1] <= (W - 1) * hop:
        raise BsedError("stitch_windows: starts must be 0, h, 2h, ... with at most the last window moved forward to the "
                        "end of the recording (window_plan's layout)")
    return s, hop


def stitch_windows(win_probs, starts, weighting="triangular"):
    """(W, Tp, C) GPU window probabilities + window starts in output frames (``window_plan``) -> (T_total, C) GPU tensor:
    every frame of the recording is the weighted mean of the windows that cover it, summed in ascending window order in
    one HIP launch without atomics (two runs give the same bits; a frame covered once is copied).  weighting:
    ``"uniform"``, or ``"triangular"`` = ``min(j + 1, Tp - j)`` for local frame j, which trusts the middle of a window more
    than its edges (one-sided GRU context, reflected audio under the STFT)."""
    if weighting not in _WEIGHTINGS:
        raise BsedError(f"stitch_windows: weighting must be one of {sorted(_WEIGHTINGS)}, got {weighting!r}")
    p = win_probs.contiguous()
    W, Tp, C = p.shape
    s, hop = _stitch_geometry(starts, Tp)
    if len(s) != W:
        raise BsedError(f"stitch_windows: {W} windows but {len(s)} starts")
    T_total = int(s[-1]) + Tp
    starts_dev = torch.as_tensor(s.astype(np.int32), device=p.device)
    out = torch.empty((T_total, C), device=p.device, dtype=torch.float32)
    L.call("bsed_stitch_windows", L.ptr(p), L.ptr(starts_dev, torch.int32), W, Tp, C, hop, T_total,
           L.CONSTANTS[_WEIGHTINGS[weighting]], L.ptr(out), L.stream())
    return out


def decode_long_gpu(mask, scale, max_len_seconds):
    """``decode_regions_gpu`` for ONE (T, C) 0/1 GPU mask with a long time axis: the same 4-tuple (clip -- all zero --,
    class, frames, seconds), the same order (class, then time) and bits, from kernels that are parallel over time
    (chunks of 64 frames; count, exclusive prefix over (class, chunk), write) instead of one thread per column."""
    mask = mask.contiguous()
    if mask.dim() != 2:
        raise BsedError(f"decode_long_gpu takes one (T, C) mask, got shape {tuple(mask.shape)}")
    T, C = mask.shape
    if T * C == 0:
        return _no_events()
    nchunks = -(-T // L.CONSTANTS["BSED_DECODE_LONG_FRAMES"])
    _, E, outs = _count_then_write(
        C * nchunks, mask.device, ("class", "frames", "seconds"),
        lambda counts: L.call("bsed_decode_long_count", L.ptr(mask), T, C, counts, L.stream()),
        lambda offsets, *ev: L.call("bsed_decode_long_write", L.ptr(mask), offsets, T, C, scale, max_len_seconds, *ev, L.stream()))
    return (np.zeros(E, np.int32), *(o[:E].cpu().numpy() for o in outs))


def gather_windows(wave, starts, win, frame_samples):
    """(n,) GPU waveform + window starts in output frames -> (W, win) clip batch, bitwise the slices
    ``wave[s * frame_samples : s * frame_samples + win]``, one HIP launch of 16-byte row moves"""
    wave = wave.contiguous()
    s = np.asarray(starts, np.int64).ravel()
    n = wave.numel()
    if len(s) == 0 or s.min() < 0 or int(s.max()) * frame_samples + win > n:
        raise BsedError(f"gather_windows: a window of {win} samples does not lie inside the recording of {n}")
    starts_dev = torch.as_tensor(s.astype(np.int32), device=wave.device)
    out = torch.empty((len(s), win), device=wave.device, dtype=torch.float32)
    L.call("bsed_gather_windows", L.ptr(wave), n, L.ptr(starts_dev, torch.int32), len(s), win, frame_samples, L.ptr(out),
           L.stream())
    return out


def detect_recording(model, wave, decoder, predictor=None, fpn=False, *, mel=None, hop_frames=None,
                     weighting="triangular", thresholds=(0.5,), median_window=1, learned_post=False,
                     classwise_median_window=None, pooling_time_ratio=4, batch_windows=64, filename=None,
                     return_probabilities=False, stage_events=None, sr=None, resample_quality=None):
    """Events of ONE whole recording.  ``wave``: mono waveform (numpy array or GPU tensor) already at ``mel.cfg.sr`` (no
    file reading here; see ``features.load_audio``) -- or, with ``sr`` given, the recording as its file holds it: int16 or
    float32, (n,) or (n, channels), at ``sr`` Hz, which ``features.Resampler(sr, mel.cfg.sr, **resample_quality)`` first
    mixes to mono and resamples in one launch (a "resample" stage in ``stage_events``; mono float32 with
    ``sr == mel.cfg.sr`` needs none and takes the ``sr=None`` route).  The resampling filter is this package's own, not
    librosa's.  ``mel``: the ``MelFrontEnd`` the model was trained with (default: the reference configuration), its ``Scaler`` attached if the model was trained on normalised features (``checkpoint.load_models(...)["scaler"]`` -> ``MelFrontEnd.set_scaler``): the windows follow the front end, there is no separate argument; ``decoder``: ``ManyHotEncoder.decode_strong`` as for ``get_predictions``.  Returns a DataFrame with
    the columns of ``get_predictions`` (event_label / onset / offset / filename; seconds from the start of the
    recording, clipped to its duration), or a list of them, one per threshold; with ``return_probabilities`` the tuple
    (that, stitched (T_total, C) GPU probabilities, per-window (W, Tp, C) GPU probabilities).

    ``window_plan`` -> ``bsed_gather_windows`` (the whole (W, win) clip batch, 1.28 MB per window) -> per chunk of
    ``batch_windows`` windows ``mel.transform`` -> ``model`` -> ``predictor`` in eval mode under no_grad, exactly the clip
    path on those windows (``predictor=None, fpn=True`` calls ``model(x, inference=True)`` as ``get_predictions`` does)
    -> ``stitch_windows`` -> ``binarize_median_gpu`` / ``binarize_median_classwise_gpu`` -> ``decode_long_gpu``.  A recording
    shorter than one window is one clip, padded as ``MelFrontEnd.transform`` pads clips.  The models' training flags are
    restored on exit; the one host sync per threshold is the event count.  ``stage_events``: a list that receives
    (stage, start event, end event) triples for tools that time the stages."""
    from .features import MelFrontEnd
    _check_form("detect_recording", predictor, fpn)
    labels = _encoder_labels(decoder, "decode_strong")
    if labels is None:
        raise BsedError("detect_recording decodes on the GPU and needs the label list: pass the bound decode_strong of a "
                        "ManyHotEncoder as decoder")
    if batch_windows < 1:
        raise BsedError(f"detect_recording: batch_windows must be at least 1, got {batch_windows}")
    if sr is None and resample_quality is not None:
        raise BsedError("detect_recording: resample_quality needs sr, the rate of the samples passed")
    if sr is not None:
        if isinstance(sr, bool) or not isinstance(sr, (int, np.integer)) or sr < 1:
            raise BsedError(f"detect_recording: sr must be the recording's rate in Hz, a positive integer, got {sr!r}")
        if not isinstance(resample_quality, (dict, type(None))) or set(resample_quality or ()) - {"rolloff", "attenuation_db"}:
            raise BsedError("detect_recording: resample_quality is a dict with the keys rolloff and / or attenuation_db, "
                            f"got {resample_quality!r}")
        from .features import Resampler, resampler
        raw_form = Resampler.form(wave)                 # dtype, shape, channels: BsedError before any GPU work
    mel = MelFrontEnd() if mel is None else mel
    cfg = mel.cfg
    rs = None
    if sr is not None:
        rs = resampler(int(sr), cfg.sr, **(resample_quality or {}))
        if rs.passes_through(wave):
            rs = None
    if rs is not None:
        n = rs.n_out(raw_form[0])                       # the resampled length, for the window plan
    else:
        wave = torch.as_tensor(np.asarray(wave, dtype=np.float32) if not isinstance(wave, torch.Tensor) else wave)
        if wave.dim() != 1 or wave.numel() == 0:
            raise BsedError(f"detect_recording takes one mono waveform (n,), got shape {tuple(wave.shape)}")
        n = wave.numel()
    starts, Tp, T_total = window_plan(n, cfg.sr, cfg.hop_size, pooling_time_ratio, cfg.max_len_seconds, hop_frames)
    if learned_post and classwise_median_window is None:
        classwise_median_window = classwise_median_windows(cfg.sr, cfg.hop_size, pooling_time_ratio)
    if rs is None:
        wave = wave.float().cuda().contiguous()
    win, frame = int(cfg.max_len_seconds * cfg.sr), cfg.hop_size * pooling_time_ratio

    def stage(name, fn):
        if stage_events is None:
            return fn()
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        out = fn()
        e.record()
        stage_events.append((name, s, e))
        return out

    with _eval_mode(model, predictor), torch.no_grad():
        if rs is not None:
            wave = stage("resample", lambda: rs(wave))
        windows = stage("front_end", lambda: wave[None] if n < win else gather_windows(wave, starts, win, frame))
        probs = []
        for i in range(0, len(starts), batch_windows):
            x = stage("front_end", lambda: mel.transform(windows[i:i + batch_windows]))
            probs.append(stage("forward", lambda: _forward(model, predictor, fpn, x)[0]))
        win_probs = probs[0] if len(probs) == 1 else torch.cat(probs)
        if tuple(win_probs.shape[:2]) != (len(starts), Tp):
            raise BsedError(f"detect_recording: the model returned {tuple(win_probs.shape)} for {len(starts)} windows "
                            f"of {Tp} output frames (pooling_time_ratio={pooling_time_ratio})")
        stitched = stage("stitch", lambda: stitch_windows(win_probs, starts, weighting))
    scale = pooling_time_ratio / (cfg.sr / cfg.hop_size)
    duration = n / cfg.sr
    dfs = []
    for t in thresholds:
        def post():
            p3 = stitched[None]
            mask = (binarize_median_classwise_gpu(p3, t, list(classwise_median_window)) if learned_post
                    else binarize_median_gpu(p3, t, median_window))
            return decode_long_gpu(mask[0], scale, duration)
        _, ev_class, _, ev_sec = stage("post", post)
        dfs.append(_event_frame(labels, ev_class, ev_sec, np.full(len(ev_class), filename, dtype=object)))
    predictions = dfs[0] if len(dfs) == 1 else dfs
    return (predictions, stitched, win_probs) if return_probabilities else predictions


# ---------------------------------------------------------------------------------------------------------------------
# Validation: threshold sweep, collar-based event counts, event F1
# ---------------------------------------------------------------------------------------------------------------------
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
        B, C = len(names), len(labels)
        index = {n: i for i, n in enumerate(names)}
        if len(index) != B:
            raise BsedError("EventReference: a clip name appears twice in the batch; scoring needs one event list per file")
        evaluated = np.zeros(B, bool)
        if groundtruth_df is None or len(groundtruth_df) == 0:
            return cls(np.zeros((B, C), np.int64), np.zeros((0, 2)), names, labels, evaluated)
        clip = np.asarray([index.get(f, -1) for f in groundtruth_df["filename"]], np.int64)
        evaluated[clip[clip >= 0]] = True
        cls_, on, off, keep, bad = _event_table(groundtruth_df, labels, ignore_unknown, clip >= 0)
        if bad is not None:
            raise BsedError(f"EventReference: event label {groundtruth_df['event_label'].iloc[bad]!r} of clip "
                            f"{names[clip[bad]]!r} is not in the label list")
        clip, cls_, on, off = clip[keep], cls_[keep], on[keep], off[keep]
        order = np.lexsort((off, on, cls_, clip))
        counts = np.bincount(clip * C + cls_, minlength=B * C).reshape(B, C)
        return cls(counts, np.stack([on[order], off[order]], 1), names, labels, evaluated)

    @classmethod
    def from_annotation_dirs(cls, names, folders, labels, ignore_unknown=False, require_annotations=False):
        """the reference of a batch from ``<folder>/<name>.txt`` (tab-separated onset / offset / event_label), the files
        ``get_predictions`` reads; a clip whose file is missing or has no row is not evaluated"""
        import pandas as pd
        dfs, _ = _read_annotations(names, folders, require_annotations)
        return cls.from_frame(pd.concat(dfs, ignore_index=True) if dfs else None, labels, names, ignore_unknown)

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
    if out is None:
        out = torch.zeros((S, C, 3), device=events.offsets.device, dtype=torch.int64)
    elif tuple(out.shape) != (S, C, 3):
        raise BsedError(f"event_counts_gpu: out must be ({S}, {C}, 3), got {tuple(out.shape)}")
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
    c = counts.detach().cpu().numpy() if isinstance(counts, torch.Tensor) else np.asarray(counts)
    if c.ndim < 2 or c.shape[-1] != 3:
        raise BsedError(f"event_f1 takes (..., C, 3) counts, got shape {c.shape}")
    c = c.astype(np.float64)

    def f(ntp, den):
        return np.divide(2.0 * ntp, den, out=np.full(den.shape, np.nan), where=den > 0)

    class_f1 = f(c[..., 0], c[..., 1] + c[..., 2])
    valid = ~np.isnan(class_f1)
    n_valid = valid.sum(-1)
    total = np.zeros(n_valid.shape)
    for k in range(class_f1.shape[-1]):                 # summed in class order, so that the value is defined to the bit
        total = total + np.where(valid[..., k], class_f1[..., k], 0.0)
    macro = np.divide(total, n_valid, out=np.full(n_valid.shape, np.nan), where=n_valid > 0)
    tot = c.sum(-2)
    return {"class_f1": class_f1, "macro": macro, "micro": f(tot[..., 0], tot[..., 1] + tot[..., 2])}


# ---------------------------------------------------------------------------------------------------------------------
# Intersection-based scoring: DTC / GTC / CTTC counts on the GPU, intersection F1, rates and PSDS on the host
# ---------------------------------------------------------------------------------------------------------------------
def _criteria(intersection, who):
    """``intersection`` argument (True or a ``(dtc, gtc, cttc)`` tuple) -> the three thresholds as floats"""
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
    if (events.B, events.C) != (reference.B, reference.C):
        raise BsedError(f"intersection_counts_gpu: the events cover {events.B} clips x {events.C} classes, the reference "
                        f"{reference.B} x {reference.C}")
    S, B, C = events.S, events.B, events.C
    dev = events.offsets.device
    if out is None:
        out = (torch.zeros((S, C, 4), device=dev, dtype=torch.int64), torch.zeros((S, C, C), device=dev, dtype=torch.int64))
    elif len(out) != 2 or tuple(out[0].shape) != (S, C, 4) or tuple(out[1].shape) != (S, C, C):
        raise BsedError(f"intersection_counts_gpu: out must be an (({S}, {C}, 4), ({S}, {C}, {C})) pair of tensors")
    for name, v in (("dtc", dtc), ("gtc", gtc), ("cttc", cttc)):
        if not 0.0 < float(v) <= 1.0:
            raise BsedError(f"intersection_counts_gpu: {name} must lie in (0, 1], got {v!r}")
    if S * B * C == 0:
        return out
    if events.total > events.seconds.shape[0] or events.offsets.numel() != S * B * C + 1:
        raise BsedError(f"intersection_counts_gpu: the event lists hold {events.seconds.shape[0]} rows and "
                        f"{events.offsets.numel()} offsets for {events.total} events in {S * B * C} groups")
    ref_off, ref_sec = reference.device()
    flags = torch.empty(events.seconds.shape[0], device=dev, dtype=torch.uint8)     # max(E, 1) bytes of scratch
    L.call("bsed_intersection_counts", L.ptr(events.offsets, torch.int32), L.ptr(events.seconds, torch.float64),
           L.ptr(ref_off, torch.int32), L.ptr(ref_sec, torch.float64), L.ptr(reference.device_evaluated(), torch.uint8),
           S, B, C, float(dtc), float(gtc), float(cttc), L.ptr(flags, torch.uint8), L.ptr(out[0], torch.int64),
           L.ptr(out[1], torch.int64), L.stream())
    return out


def _host_counts(a, last, who):
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    if a.ndim < 2 or a.shape[-1] != last:
        raise BsedError(f"{who}, got shape {a.shape}")
    return a


def intersection_f1(acc):
    """(..., C, 4) integer counts (Ntp, Nfp, Nsys, Nref) -> dict of float64 numpy arrays: ``class_f1`` (..., C) and ``macro``
    (...).  Per class F = 2 Ntp / (2 Ntp + Nfp + (Nref - Ntp)); F is NaN where Nref == 0 -- psds_eval's rule: a class
    without reference events is left out of the average even when it is predicted.  That DIFFERS from ``event_f1``, whose
    F is NaN only where the class neither occurs nor is predicted (and 0 where it is predicted but does not occur).
    ``macro`` is the mean over the classes whose F is not NaN, summed in class order (NaN if there is none)."""
    c = _host_counts(acc, 4, "intersection_f1 takes (..., C, 4) counts").astype(np.float64)
    ntp, nfp, nref = c[..., 0], c[..., 1], c[..., 3]
    class_f1 = np.divide(2.0 * ntp, 2.0 * ntp + nfp + (nref - ntp), out=np.full(ntp.shape, np.nan), where=nref > 0)
    valid = ~np.isnan(class_f1)
    n_valid = valid.sum(-1)
    total = np.zeros(n_valid.shape)
    for k in range(class_f1.shape[-1]):                 # summed in class order, so that the value is defined to the bit
        total = total + np.where(valid[..., k], class_f1[..., k], 0.0)
    return {"class_f1": class_f1, "macro": np.divide(total, n_valid, out=np.full(n_valid.shape, np.nan), where=n_valid > 0)}


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


def _frame_lists(dfs, labels, names, who):
    """prediction frames (one per operating point; event_label / onset / offset / filename) -> ``EventLists`` over
    ``names`` x ``labels``: rows grouped by (clip, class) in frame order; rows of other files are ignored, rows with a
    NaN time dropped, a label outside ``labels`` raises"""
    index = {n: i for i, n in enumerate(names)}
    B, C = len(names), len(labels)
    counts, secs = np.zeros((len(dfs), B, C), np.int64), []
    for s, df in enumerate(dfs):
        if df is None or len(df) == 0:
            continue
        clip = np.asarray([index.get(f, -1) for f in df["filename"]], np.int64)
        k, on, off, keep, bad = _event_table(df, labels, False, clip >= 0)
        if bad is not None:
            raise BsedError(f"{who}: estimated event label {df['event_label'].iloc[bad]!r} is not in the label list")
        group = (clip * C + k)[keep]
        order = np.argsort(group, kind="stable")
        counts[s] = np.bincount(group, minlength=B * C).reshape(B, C)
        secs.append(np.stack([on[keep][order], off[keep][order]], 1))
    return EventLists.from_host(counts, np.concatenate(secs) if secs else np.zeros((0, 2)))


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
    ``intersection``, else None."""

    def __init__(self, thresholds, counts, labels, predictions=None, groundtruth_df=None, tagging=None, intersection=None):
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


def validate(model, dataloader, decoder, predictor=None, fpn=False, thresholds=(0.5,), median_window=1, learned_post=False,
             t_collar=0.2, percentage_of_length=0.2, pooling_time_ratio=1, sr=32000, hop_size=255, max_len_seconds=10.0,
             classwise_median_window=None, return_predictions=False, require_annotations=False, ignore_unknown=False,
             tagging_thresholds=None, intersection=None):
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
    counts ``max_len_seconds`` in the total duration.  With None the pass launches and returns what it did without it."""
    import pandas as pd
    _check_form("validate", predictor, fpn)
    criteria = None if intersection is None or intersection is False else _criteria(intersection, "validate")
    isect_acc, ref_duration, n_evaluated = None, None, 0
    labels = _encoder_labels(decoder, "decode_strong")
    if labels is None:
        raise BsedError("validate decodes and scores on the GPU and needs the label list: pass the bound decode_strong of a "
                        "ManyHotEncoder as decoder")
    thresholds = [float(t) for t in thresholds]
    if learned_post and classwise_median_window is None:
        classwise_median_window = classwise_median_windows(sr, hop_size, pooling_time_ratio)
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
            dfs, _ = _read_annotations(names, folders, require_annotations)
            reference = EventReference.from_frame(pd.concat(dfs, ignore_index=True) if dfs else None, labels[:C], names,
                                                  ignore_unknown)
            event_counts_gpu(events, reference, t_collar, percentage_of_length, out=acc)
            if criteria is not None:
                isect_acc = intersection_counts_gpu(events, reference, *criteria, out=isect_acc)
                durations = reference.class_durations()
                ref_duration = durations if ref_duration is None else ref_duration + durations
                n_evaluated += int(reference.evaluated.sum())
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
    return ValidationResult(thresholds, acc.cpu().numpy(), labels[:acc.shape[1]], predictions, groundtruth_df, tagging, isect)


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

    def columns(df, what):
        if df is None or len(df) == 0:
            return np.zeros(0, np.int64), np.zeros(0), np.zeros(0)
        k, on, off, keep, bad = _event_table(df, labels, ignore_unknown and what == "reference")
        if bad is not None:
            raise BsedError(f"score_recording: {what} event label {df['event_label'].iloc[bad]!r} is not in the label list")
        return k[keep], on[keep], off[keep]

    rk, ron, roff = columns(groundtruth_df, "reference")
    order = np.lexsort((roff, ron, rk))
    rk, ron, roff = rk[order], ron[order], roff[order]
    gap = 2.0 * float(t_collar) + _SEGMENT_SLACK
    piece = np.zeros(len(rk), np.int64)                 # piece index of every reference event inside its class
    starts = []                                         # per class: first onset of every piece
    for c in range(C):
        idx = np.nonzero(rk == c)[0]
        new = np.concatenate([[True], np.diff(ron[idx]) > gap]) if len(idx) else np.zeros(0, bool)
        piece[idx] = np.cumsum(new) - 1
        starts.append(ron[idx][new])
    Bp = max([1] + [len(s) for s in starts])
    ref_counts = np.bincount(piece * C + rk, minlength=Bp * C).reshape(Bp, C)
    rorder = np.lexsort((roff, ron, rk, piece))
    names = [f"piece {i}" for i in range(Bp)]
    reference = EventReference(ref_counts, np.stack([ron[rorder], roff[rorder]], 1), names, labels)
    if ref_counts.max(initial=0) > MATCH_MAX_REF:
        b, c = np.unravel_index(int(np.argmax(ref_counts)), ref_counts.shape)
        raise BsedError(f"score_recording: {int(ref_counts[b, c])} reference events of class {labels[c]!r} from "
                        f"{starts[c][b]:.3f} s on follow each other within {gap:.3f} s; the matcher takes at most "
                        f"{MATCH_MAX_REF} per such run")
    counts = np.zeros((len(dfs), Bp, C), np.int64)
    secs = []
    for s, df in enumerate(dfs):
        ek, eon, eoff = columns(df, "estimated")
        ep = np.zeros(len(ek), np.int64)
        for c in range(C):
            idx = np.nonzero(ek == c)[0]
            if len(idx) and len(starts[c]):
                ep[idx] = np.maximum(np.searchsorted(starts[c] - float(t_collar) - _SEGMENT_SLACK / 2, eon[idx], "right") - 1, 0)
        o = np.lexsort((eoff, eon, ek, ep))
        counts[s] = np.bincount(ep * C + ek, minlength=Bp * C).reshape(Bp, C)
        secs.append(np.stack([eon[o], eoff[o]], 1))
    return counts, np.concatenate(secs) if secs else np.zeros((0, 2)), reference


def score_recording(events_df, groundtruth_df, labels, t_collar=0.2, percentage_of_length=0.2, ignore_unknown=False,
                    intersection=None, duration=None):
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
    the recording's length in seconds, which only ``PsdsResult.psds`` and the false-positive rates need."""
    counts, seconds, reference = recording_problem(events_df, groundtruth_df, labels, t_collar, ignore_unknown)
    events = EventLists.from_host(counts, seconds)
    event_counts = event_counts_gpu(events, reference, t_collar, percentage_of_length).cpu().numpy()
    if intersection is None or intersection is False:
        return event_counts
    criteria = _criteria(intersection, "score_recording")
    labels = list(labels)
    dfs = [df.assign(filename="recording") for df in (events_df if isinstance(events_df, (list, tuple)) else [events_df])]
    gt = None if groundtruth_df is None or len(groundtruth_df) == 0 else groundtruth_df.assign(filename="recording")
    whole = EventReference.from_frame(gt, labels, ["recording"], ignore_unknown)
    whole.evaluated[:] = True                           # a recording without a reference event is still scored
    acc, ct = intersection_counts_gpu(_frame_lists(dfs, labels, ["recording"], "score_recording"), whole, *criteria)
    return event_counts, PsdsResult(acc, ct, whole.class_durations(), duration, labels, None, criteria)


# ---------------------------------------------------------------------------------------------------------------------
# Clip-level tagging: weak F1 over a threshold sweep, pseudo weak labels
# ---------------------------------------------------------------------------------------------------------------------
TAG_MASK_MAX_CLASSES = 64


class TagThresholds:
    """The thresholds of a tagging sweep: ``(S)`` numbers applied to every class, or ``(S, C)`` rows of per-class
    thresholds (one row is the reference's ``thresholds_`` list, src/evaluation_measures.py:400-406).  ``host``: a list of
    floats, or of lists of floats; ``device``: the float32 GPU tensor the kernel compares with (scores are float32, and
    numpy compares a float32 array with a Python number in float32 too); ``per_class``; ``S``; ``C`` (None when global)."""

    def __init__(self, thresholds):
        if isinstance(thresholds, torch.Tensor):
            thresholds = thresholds.detach().cpu().numpy()
        a = np.asarray(thresholds, dtype=np.float64)
        if a.ndim not in (1, 2) or a.size == 0:
            raise BsedError(f"tagging thresholds must be (S) numbers or (S, C) per-class rows, got shape {a.shape}")
        self.per_class, self.S = a.ndim == 2, a.shape[0]
        self.C = a.shape[1] if self.per_class else None
        self.host = a.tolist()
        self._array, self._dev = np.ascontiguousarray(a.astype(np.float32)), None

    @property
    def device(self):
        if self._dev is None:
            self._dev = torch.from_numpy(self._array).cuda()
        return self._dev


def _tag_form(x, what):
    """(B,C) or (B,T,C) tensor / array -> (contiguous float32 GPU tensor, T or 0 for the 2-D form)"""
    if not isinstance(x, torch.Tensor):
        x = torch.as_tensor(np.asarray(x))
    if x.dim() not in (2, 3):
        raise BsedError(f"{what} must be (B, C) or (B, T, C), got shape {tuple(x.shape)}")
    if x.dim() == 3 and x.shape[1] == 0:
        raise BsedError(f"{what}: a (B, T, C) tensor needs at least one frame, got shape {tuple(x.shape)}")
    x = x.detach().to(device="cuda", dtype=torch.float32).contiguous()
    return x, (x.shape[1] if x.dim() == 3 else 0)


def tag_counts_gpu(scores, targets, thresholds, out=None):
    """Weak scores x targets x a threshold sweep -> (S,C,4) int64 GPU tensor of (tp, fp, fn, tn) summed over the clips,
    ADDED into ``out`` when given (the accumulator of a validation pass; allocated and zeroed when None).  One HIP launch
    (``bsed_tag_counts``), no host sync.  ``scores``: (B,C), or (B,T,C) from a model that only predicts strong outputs,
    reduced by its maximum over time; ``targets``: (B,C), used as given, or (B,T,C), reduced by its maximum over time and
    binarised with ``> 0.5`` -- the reference's forms (src/evaluation_measures.py:386-398); ``thresholds``: (S) numbers,
    (S,C) per-class rows, or a ``TagThresholds``.  ``est = score > threshold`` (a NaN score is 0); the four counts are
    ``intermediate_at_measures``' compares (:442-446) on the float target value, so a row of -1 (``encode_weak("empty")``)
    counts as it does there."""
    thr = thresholds if isinstance(thresholds, TagThresholds) else TagThresholds(thresholds)
    x, Ts = _tag_form(scores, "tag_counts_gpu: scores")
    y, Tt = _tag_form(targets, "tag_counts_gpu: targets")
    B, C = x.shape[0], x.shape[-1]
    if (y.shape[0], y.shape[-1]) != (B, C):
        raise BsedError(f"tag_counts_gpu: scores cover {B} clips x {C} classes, targets {y.shape[0]} x {y.shape[-1]}")
    if C == 0:
        raise BsedError("tag_counts_gpu: no class")
    if thr.per_class and thr.C != C:
        raise BsedError(f"tag_counts_gpu: per-class thresholds have {thr.C} columns, the scores {C} classes")
    if out is None:
        out = torch.zeros((thr.S, C, 4), device=x.device, dtype=torch.int64)
    elif tuple(out.shape) != (thr.S, C, 4):
        raise BsedError(f"tag_counts_gpu: out must be ({thr.S}, {C}, 4), got {tuple(out.shape)}")
    L.call("bsed_tag_counts", L.ptr(x), Ts, L.ptr(y), Tt, L.ptr(thr.device), int(thr.per_class), thr.S, B, C,
           L.ptr(out, torch.int64), L.stream())
    return out


def tag_masks_gpu(scores, threshold=0.5, class_thresholds=None, out=None, row_offset=0, nonempty=None):
    """Weak scores (B,C) or (B,T,C) -> ``(out, nonempty)``: ``out`` (N) int64 GPU buffer whose rows ``row_offset ..
    row_offset + B`` receive one bit mask per clip (bit c set when class c is on; read it as uint64), ``nonempty`` a
    one-element int64 GPU counter the number of clips with any bit is ADDED to.  Both are allocated (N = B, zero) when
    None.  ``class_thresholds``: a list of C per-class thresholds in place of ``threshold``.  At most 64 classes."""
    x, Ts = _tag_form(scores, "tag_masks_gpu: scores")
    B, C = x.shape[0], x.shape[-1]
    cls = None
    if class_thresholds is not None:
        cls = torch.tensor([float(t) for t in class_thresholds], dtype=torch.float32).cuda()
        if cls.numel() != C:
            raise BsedError(f"tag_masks_gpu: {cls.numel()} class thresholds for {C} classes")
    if out is None:
        out = torch.zeros(row_offset + B, device=x.device, dtype=torch.int64)
    if nonempty is None:
        nonempty = torch.zeros(1, device=x.device, dtype=torch.int64)
    if out.dim() != 1 or nonempty.numel() != 1:
        raise BsedError("tag_masks_gpu: out is an (N) int64 buffer and nonempty a one-element int64 counter")
    L.call("bsed_tag_masks", L.ptr(x), Ts, L.ptr(cls), float(threshold), B, C, int(row_offset), out.numel(),
           L.ptr(out, torch.int64), L.ptr(nonempty, torch.int64), L.stream())
    return out, nonempty


def tag_f1(counts):
    """(..., C, 4) integer counts (tp, fp, fn, tn) -> (..., C) float64 per-class F1 = 2 tp / (2 tp + fp + fn), and 0 where
    that denominator is 0 (reference src/evaluation_measures.py:423-425)."""
    c = counts.detach().cpu().numpy() if isinstance(counts, torch.Tensor) else np.asarray(counts)
    if c.ndim < 2 or c.shape[-1] != 4:
        raise BsedError(f"tag_f1 takes (..., C, 4) counts, got shape {c.shape}")
    c = c.astype(np.float64)
    num, den = 2.0 * c[..., 0], 2.0 * c[..., 0] + c[..., 1] + c[..., 2]
    return np.divide(num, den, out=np.zeros(den.shape), where=den != 0)


class TaggingResult:
    """``validate_weak``'s return value: ``thresholds`` (S numbers, or S per-class rows), ``counts`` (S,C,4) int64 numpy
    (tp, fp, fn, tn), ``class_f1`` (S,C) and ``macro_f1`` (S) float64 (the mean over the classes, the number the reference
    keeps ``baseline_best`` by), ``best_index`` / ``best_threshold`` / ``best_macro_f1`` (highest macro F1, ties to the lowest
    threshold -- the rule of ``ValidationResult``), ``class_thresholds``: per class the threshold with the highest class
    F1, ties to the lowest, a plain list ready to be passed back as the reference's ``thresholds_``.  The F values are
    compared exactly, as fractions of the integer counts, never as rounded floats."""

    def __init__(self, thresholds, counts, labels=None):
        self.thresholds = thresholds.host if isinstance(thresholds, TagThresholds) else [
            list(map(float, t)) if np.ndim(t) else float(t) for t in thresholds]
        self.counts = np.asarray(counts, np.int64)
        if self.counts.ndim != 3 or self.counts.shape[2] != 4 or self.counts.shape[0] != len(self.thresholds):
            raise BsedError(f"TaggingResult: counts must be ({len(self.thresholds)}, C, 4), got {self.counts.shape}")
        S, C, _ = self.counts.shape
        self.labels = None if labels is None else list(labels)
        self.class_f1 = tag_f1(self.counts)
        self.macro_f1 = self.class_f1.mean(1) if C else np.zeros(S)

        def frac(s, c):
            tp, fp, fn, _ = (int(v) for v in self.counts[s, c])
            den = 2 * tp + fp + fn
            return Fraction(2 * tp, den) if den else Fraction(0)

        def at(s, c):                                   # the threshold class c sees in sweep row s
            t = self.thresholds[s]
            return t[c] if isinstance(t, list) else t

        exact = [[frac(s, c) for c in range(C)] for s in range(S)]
        total = [sum(row, Fraction(0)) for row in exact]            # macro F1 * C, exactly
        # highest F first; among equals the lowest threshold, then the earliest row
        self.best_index = min(range(S), key=lambda s: (-total[s], self.thresholds[s], s))
        self.best_threshold = self.thresholds[self.best_index]
        self.best_macro_f1 = float(self.macro_f1[self.best_index])
        self.class_best_index = [min(range(S), key=lambda s: (-exact[s][c], at(s, c), s)) for c in range(C)]
        self.class_thresholds = [at(s, c) for c, s in enumerate(self.class_best_index)]


def _loader_targets(y, who):
    if y is None:
        raise BsedError(f"{who} scores against the loader's own targets, and the loader yielded None")
    return y if isinstance(y, torch.Tensor) else torch.as_tensor(np.asarray(y))


def validate_weak(model, dataloader, predictor=None, trained=False, fpn=False, thresholds=(0.5,), class_thresholds=None):
    """One pass of clip-level (weak) scoring on the GPU -> ``TaggingResult``.  The eval-mode forward of ``get_predictions``
    on the same ``(((input, ema_input), target), paths)`` batches; the weak output of every batch is scored against the
    loader's own ``target`` over ALL ``thresholds`` in one launch (``tag_counts_gpu``), the counts are accumulated on the
    device and read once at the end.  ``class_thresholds``: a list of per-class thresholds scored INSTEAD of the sweep
    (one row: the reference's ``thresholds_``).  ``trained=True``: ``model(x)`` is the tagger itself (the reference's
    ``pred_weak = torch_model(batch_x)``); a ``(strong, weak)`` return, as ``CRNN_pred`` gives, contributes its weak part.
    Training flags are restored on exit."""
    _check_form("validate_weak", predictor, fpn, trained)
    thr = TagThresholds([list(class_thresholds)] if class_thresholds is not None else list(thresholds))
    acc = None
    with _eval_mode(model, predictor):
        for x, target, _paths, _, _ in _batches(dataloader):
            pred_weak = _forward(model, predictor, fpn, x, trained, weak=True)[1]
            acc = tag_counts_gpu(pred_weak, _loader_targets(target, "validate_weak"), thr, out=acc)
    if acc is None:
        raise BsedError("validate_weak: the dataloader yielded no batch")
    return TaggingResult(thr, acc.cpu().numpy())        # the one read-back of the pass


def get_f_measure_by_class(torch_model, nb_tags, dataloader_, thresholds_=None, trained=False, predictor=None):
    """The reference's signature and return value (src/evaluation_measures.py:346-427): the per-class weak F1 as a float64
    array of ``nb_tags``, at 0.5 or at the per-class list ``thresholds_``; counted on the GPU by ``validate_weak``."""
    if thresholds_ is not None and type(thresholds_) is not list:
        raise BsedError("get_f_measure_by_class: thresholds_ is a list of per-class thresholds (the reference asserts it)")
    res = validate_weak(torch_model, dataloader_, predictor=predictor, trained=trained, class_thresholds=thresholds_)
    if res.counts.shape[1] != nb_tags:
        raise BsedError(f"get_f_measure_by_class: the model returned {res.counts.shape[1]} classes, nb_tags is {nb_tags}")
    return res.class_f1[0].copy()


def pseudo_label_frame(masks, filenames, labels):
    """(N) uint64 bit masks + the N file names + the label list -> the DataFrame [filename, event_labels] the reference
    writes (src/audio_tagging_inference.py:304-316): ``event_labels`` the on labels in label-index order joined with ",",
    clips without a label left out, rows in the order given.  The strings are built once per DISTINCT mask."""
    import pandas as pd
    masks = np.ascontiguousarray(masks).view(np.uint64).ravel()
    if len(masks) != len(filenames):
        raise BsedError(f"pseudo_label_frame: {len(masks)} masks for {len(filenames)} file names")
    uniq, inverse = np.unique(masks, return_inverse=True)
    if len(uniq) and int(uniq.max()) >> len(labels):
        raise BsedError(f"pseudo_label_frame: a mask has a bit beyond the {len(labels)} labels")
    text = np.asarray([",".join(l for c, l in enumerate(labels) if (int(m) >> c) & 1) for m in uniq], dtype=object)
    keep = masks != 0
    return pd.DataFrame({"filename": np.asarray(list(filenames), dtype=object)[keep],
                         "event_labels": text[inverse.ravel()][keep] if len(uniq) else np.zeros(0, object)},
                        columns=["filename", "event_labels"])


def pseudo_label(model, dataloader, decoder, predictor=None, trained=False, fpn=False, threshold=0.5,
                 class_thresholds=None, save_path=None):
    """Pseudo weak labels of an (unlabelled) pool -> DataFrame [filename, event_labels], the file ``PseudoWeakDataset``
    reads (reference src/audio_tagging_inference.py:289-316).  The forward forms of ``validate_weak``; every batch's weak
    output is thresholded at ``threshold`` (or the per-class list ``class_thresholds``) into one bit mask per clip
    (``bsed_tag_masks``), the masks stay in ONE device buffer for the whole pool and are read once, 8 bytes per clip.
    ``decoder``: the bound ``decode_weak`` of a ManyHotEncoder (its label list names the bits); ``filename`` is the path
    string the loader yielded; clips without a label are left out; row order is loader order.  ``save_path``: also
    written as ``to_csv(index=False, sep="\\t")``.  Training flags are restored on exit."""
    _check_form("pseudo_label", predictor, fpn, trained)
    labels = _encoder_labels(decoder, "decode_weak")
    if labels is None:
        raise BsedError("pseudo_label thresholds on the GPU and needs the label list: pass the bound decode_weak of a "
                        "ManyHotEncoder as decoder")
    try:
        capacity = max(int(len(dataloader.dataset)), 1)             # a torch DataLoader knows the pool's size
    except (AttributeError, TypeError):
        capacity = 4096
    buf = nonempty = None
    filenames = []
    with _eval_mode(model, predictor):
        for x, _target, paths, _, _ in _batches(dataloader):
            pred_weak = _forward(model, predictor, fpn, x, trained, weak=True)[1]
            B, C = pred_weak.shape[0], pred_weak.shape[-1]
            if C > len(labels):
                raise BsedError(f"pseudo_label: the model returned {C} classes, the decoder has {len(labels)} labels")
            if len(paths) != B:
                raise BsedError(f"pseudo_label: {B} clips but {len(paths)} paths in one batch")
            n = len(filenames)
            if buf is None:
                buf = torch.zeros(max(capacity, B), device=pred_weak.device, dtype=torch.int64)
                nonempty = torch.zeros(1, device=pred_weak.device, dtype=torch.int64)
            elif n + B > buf.numel():                   # an unsized loader: grow on the device, nothing is read back
                grown = torch.zeros(max(2 * buf.numel(), n + B), device=buf.device, dtype=torch.int64)
                grown[:n] = buf[:n]
                buf = grown
            tag_masks_gpu(pred_weak, threshold, class_thresholds, out=buf, row_offset=n, nonempty=nonempty)
            filenames += [str(p) for p in paths]
    if buf is None:
        raise BsedError("pseudo_label: the dataloader yielded no batch")
    masks = buf[:len(filenames)].cpu().numpy().view(np.uint64)      # the one read-back of the pool
    if int(nonempty.item()) != int(np.count_nonzero(masks)):
        raise BsedError(f"pseudo_label: the device counted {int(nonempty.item())} labelled clips, the masks hold "
                        f"{int(np.count_nonzero(masks))}")
    df = pseudo_label_frame(masks, filenames, labels)
    if save_path is not None:
        if os.path.dirname(save_path):
            os.makedirs(os.path.dirname(save_path), exist_ok=True)
        df.to_csv(save_path, index=False, sep="\t")
    return df
