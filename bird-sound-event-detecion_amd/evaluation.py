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
assembled without a per-clip Python loop.  Metric values (sed_eval / psds_eval) stay external.

  detect_recording  <- no counterpart in the reference, which cuts recordings into 10 s clips offline
                       (src/data/preprocess.py:176-229) and only ever sees clips: one whole recording -> overlapping
                       clip-sized windows on the recording's frame grid (``window_plan``, ``bsed_gather_windows``) -> the clip
                       path above -> one (T_total, C) time line (``stitch_windows``) -> threshold / median / contiguous
                       regions decoded in parallel over time (``decode_long_gpu``) -> events in seconds of the recording.
"""
import math
import os

import numpy as np
import torch

from . import _lib as L
from ._lib import BsedError


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
        return (np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros((0, 2), np.int32), np.zeros((0, 2), np.float64))
    counts = torch.empty(B * C, device=mask.device, dtype=torch.int32)
    L.call("bsed_decode_count", L.ptr(mask), B, T, C, L.ptr(counts, torch.int32), L.stream())
    csum = torch.cumsum(counts, 0, dtype=torch.int32)
    offsets = (csum - counts).contiguous()
    E = int(csum[-1])                                   # the one host sync of the decode: the list length
    ev_clip = torch.empty(max(E, 1), device=mask.device, dtype=torch.int32)
    ev_class = torch.empty(max(E, 1), device=mask.device, dtype=torch.int32)
    ev_frames = torch.empty((max(E, 1), 2), device=mask.device, dtype=torch.int32)
    ev_seconds = torch.empty((max(E, 1), 2), device=mask.device, dtype=torch.float64)
    if E:
        L.call("bsed_decode_write", L.ptr(mask), L.ptr(offsets, torch.int32), B, T, C, scale,
               max_len_seconds, L.ptr(ev_clip, torch.int32), L.ptr(ev_class, torch.int32), L.ptr(ev_frames, torch.int32),
               L.ptr(ev_seconds, torch.float64), L.stream())
    return (ev_clip[:E].cpu().numpy(), ev_class[:E].cpu().numpy(), ev_frames[:E].cpu().numpy(),
            ev_seconds[:E].cpu().numpy())


def _decoder_labels(decoder):
    """label list of the ManyHotEncoder whose bound ``decode_strong`` was passed as ``decoder`` (the reference's call
    sites pass ``many_hot_encoder.decode_strong``, src/main_baseline.py:1010-1032), or None for any other callable"""
    owner = getattr(decoder, "__self__", None)
    if owner is not None and getattr(decoder, "__name__", "") == "decode_strong" and hasattr(owner, "labels"):
        return list(owner.labels)
    return None


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
    if predictor is None and not fpn:
        raise NotImplementedError("get_predictions(predictor=None, fpn=False) is the reference's seg_index call of a model "
                                  "class outside the hot path; pass predictor=... or a self-contained model with fpn=True")
    if learned_post and classwise_median_window is None:
        classwise_median_window = classwise_median_windows(sr, hop_size, pooling_time_ratio)
    was_training = (model.training, predictor.training if predictor is not None else False)
    model.eval()
    if predictor is not None:
        predictor.eval()
    labels = _decoder_labels(decoder)
    scale = pooling_time_ratio / (sr / hop_size)
    frames = {t: [] for t in thresholds}
    filename_list, annotation_folder_list = [], []
    for i, (((input_data, _ema), _target), paths) in enumerate(dataloader):
        names = [os.path.splitext(os.path.basename(p))[0] for p in paths]
        folders = [os.path.join(os.path.dirname(os.path.dirname(p)), "annotation") for p in paths]
        with torch.no_grad():
            x = torch.as_tensor(input_data).float().cuda()
            if predictor is not None:
                encoded_x, feature_out = model(x)
                pred_strong, _ = predictor(encoded_x, inference=fpn)
            else:
                pred_strong, feature_out = model(x, inference=True)[0], None
        if saved_feature_dir is not None and feature_out is not None:
            np.save(os.path.join(saved_feature_dir, f"{i}"), feature_out.cpu().numpy())
        for t in thresholds:
            mask = (binarize_median_classwise_gpu(pred_strong, t, list(classwise_median_window)) if learned_post
                    else binarize_median_gpu(pred_strong, t, median_window))
            if labels is not None:
                ev_clip, ev_class, _, ev_sec = decode_regions_gpu(mask, scale, max_len_seconds)
                frames[t].append(pd.DataFrame({"event_label": np.asarray(labels, dtype=object)[ev_class],
                                               "onset": ev_sec[:, 0], "offset": ev_sec[:, 1],
                                               "filename": np.asarray(names, dtype=object)[ev_clip]}))
            else:
                # a caller-supplied decoder function can only run on the host, clip by clip
                rows = []
                for j, m in enumerate(mask.cpu().numpy()):
                    for lab, on, off in decoder(m):
                        rows.append({"event_label": lab, "onset": float(np.clip(on * scale, 0, max_len_seconds)),
                                     "offset": float(np.clip(off * scale, 0, max_len_seconds)), "filename": names[j]})
                frames[t].append(pd.DataFrame(rows, columns=["event_label", "onset", "offset", "filename"]))
        filename_list += names
        annotation_folder_list += folders
    model.train(was_training[0])
    if predictor is not None:
        predictor.train(was_training[1])
    cols = ["event_label", "onset", "offset", "filename"]
    dfs = [pd.concat(frames[t], ignore_index=True)[cols] if frames[t] else pd.DataFrame(columns=cols)
           for t in thresholds]

    # ground-truth and duration frames (reference :226-247): first occurrence of every file name, its annotation file
    # next to the features, duration 10
    seen = {}
    for name, folder in zip(filename_list, annotation_folder_list):
        seen.setdefault(name, folder)
    duration_df = pd.DataFrame(list(seen.keys()), columns=["filename"])
    duration_df["duration"] = 10
    groundtruth_df = None
    gts, n_found = [], 0
    for name, folder in seen.items():
        path = os.path.join(folder, name + ".txt")
        if not os.path.exists(path):
            if require_annotations:
                raise FileNotFoundError(f"get_predictions: annotation file {path} is missing (the reference reads "
                                        "annotation/<name>.txt next to wav/<name>.npy)")
            continue                                    # unlabelled clip: predictions only
        n_found += 1
        df = pd.read_csv(path, sep="\t")
        df["filename"] = name
        if len(df):
            gts.append(df)
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
        return (np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros((0, 2), np.int32), np.zeros((0, 2), np.float64))
    nchunks = -(-T // L.CONSTANTS["BSED_DECODE_LONG_FRAMES"])
    counts = torch.empty(C * nchunks, device=mask.device, dtype=torch.int32)
    L.call("bsed_decode_long_count", L.ptr(mask), T, C, L.ptr(counts, torch.int32), L.stream())
    csum = torch.cumsum(counts, 0, dtype=torch.int32)
    offsets = (csum - counts).contiguous()
    E = int(csum[-1])                                   # the one host sync of the decode: the list length
    ev_class = torch.empty(max(E, 1), device=mask.device, dtype=torch.int32)
    ev_frames = torch.empty((max(E, 1), 2), device=mask.device, dtype=torch.int32)
    ev_seconds = torch.empty((max(E, 1), 2), device=mask.device, dtype=torch.float64)
    if E:
        L.call("bsed_decode_long_write", L.ptr(mask), L.ptr(offsets, torch.int32), T, C, scale, max_len_seconds,
               L.ptr(ev_class, torch.int32), L.ptr(ev_frames, torch.int32), L.ptr(ev_seconds, torch.float64), L.stream())
    return (np.zeros(E, np.int32), ev_class[:E].cpu().numpy(), ev_frames[:E].cpu().numpy(), ev_seconds[:E].cpu().numpy())


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
    librosa's.  ``mel``: the ``MelFrontEnd`` the model was trained with (default: the reference configuration); ``decoder``: ``ManyHotEncoder.decode_strong`` as for ``get_predictions``.  Returns a DataFrame with
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
    import pandas as pd
    from .features import MelFrontEnd
    if predictor is None and not fpn:
        raise NotImplementedError("detect_recording(predictor=None, fpn=False): pass predictor=... or a self-contained "
                                  "model with fpn=True (see get_predictions)")
    labels = _decoder_labels(decoder)
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

    def forward(x):
        if predictor is not None:
            return predictor(model(x)[0], inference=fpn)[0]
        return model(x, inference=True)[0]

    was_training = (model.training, predictor.training if predictor is not None else False)
    model.eval()
    if predictor is not None:
        predictor.eval()
    try:
        with torch.no_grad():
            if rs is not None:
                wave = stage("resample", lambda: rs(wave))
            windows = stage("front_end", lambda: wave[None] if n < win else gather_windows(wave, starts, win, frame))
            probs = []
            for i in range(0, len(starts), batch_windows):
                x = stage("front_end", lambda: mel.transform(windows[i:i + batch_windows]))
                probs.append(stage("forward", lambda: forward(x)))
            win_probs = probs[0] if len(probs) == 1 else torch.cat(probs)
            if tuple(win_probs.shape[:2]) != (len(starts), Tp):
                raise BsedError(f"detect_recording: the model returned {tuple(win_probs.shape)} for {len(starts)} windows "
                                f"of {Tp} output frames (pooling_time_ratio={pooling_time_ratio})")
            stitched = stage("stitch", lambda: stitch_windows(win_probs, starts, weighting))
    finally:
        model.train(was_training[0])
        if predictor is not None:
            predictor.train(was_training[1])
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
        dfs.append(pd.DataFrame({"event_label": np.asarray(labels, dtype=object)[ev_class], "onset": ev_sec[:, 0],
                                 "offset": ev_sec[:, 1], "filename": np.full(len(ev_class), filename, dtype=object)},
                                columns=["event_label", "onset", "offset", "filename"]))
    predictions = dfs[0] if len(dfs) == 1 else dfs
    return (predictions, stitched, win_probs) if return_probabilities else predictions
