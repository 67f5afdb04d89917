"""Whole-recording detection.  No counterpart in the reference, which cuts recordings into 10 s clips offline
(src/data/preprocess.py:176-229) and only ever sees clips: one whole recording -> overlapping clip-sized windows on the
recording's frame grid (``window_plan``, ``bsed_gather_windows``) -> the clip path -> one (T_total, C) time line
(``stitch_windows``) -> threshold / median / contiguous regions decoded in parallel over time (``decode_long_gpu``) ->
events in seconds of the recording."""
import math

import numpy as np
import torch

from .. import _lib as L
from .._lib import BsedError
from ._common import _check_form, _count_then_write, _eval_mode, _event_frame, _forward, _no_events, _required_labels
from .clips import _learned_windows, _threshold_mask


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


def _recording_input(wave, sr, resample_quality, mel):
    """``detect_recording``'s ``wave`` / ``sr`` / ``resample_quality`` / ``mel`` arguments, checked on the host before any
    GPU work -> ``(wave, resampler, n, mel)``: with a resampler the samples as they were passed, to be resampled to ``n``
    samples, else (resampler None) the mono float32 waveform of ``n`` samples as a tensor; ``mel``: the front end, the
    reference configuration's when None was passed (made only once the arguments before it are known to be good)"""
    from ..features import MelFrontEnd
    if sr is None and resample_quality is not None:
        raise BsedError("detect_recording: resample_quality needs sr, the rate of the samples passed")
    if sr is not None:
        if isinstance(sr, bool) or not isinstance(sr, (int, np.integer)) or sr < 1:
            raise BsedError(f"detect_recording: sr must be the recording's rate in Hz, a positive integer, got {sr!r}")
        if not isinstance(resample_quality, (dict, type(None))) or set(resample_quality or ()) - {"rolloff", "attenuation_db"}:
            raise BsedError("detect_recording: resample_quality is a dict with the keys rolloff and / or attenuation_db, "
                            f"got {resample_quality!r}")
        from ..features import Resampler, resampler
        raw_form = Resampler.form(wave)                 # dtype, shape, channels: BsedError before any GPU work
    mel = MelFrontEnd() if mel is None else mel
    rs = None
    if sr is not None:
        rs = resampler(int(sr), mel.cfg.sr, **(resample_quality or {}))
        if rs.passes_through(wave):
            rs = None
    if rs is not None:
        return wave, rs, rs.n_out(raw_form[0]), mel     # the resampled length, for the window plan
    wave = torch.as_tensor(np.asarray(wave, dtype=np.float32) if not isinstance(wave, torch.Tensor) else wave)
    if wave.dim() != 1 or wave.numel() == 0:
        raise BsedError(f"detect_recording takes one mono waveform (n,), got shape {tuple(wave.shape)}")
    return wave, None, wave.numel(), mel


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
    _check_form("detect_recording", predictor, fpn)
    labels = _required_labels(decoder, "decode_strong", "detect_recording", "decodes")
    if batch_windows < 1:
        raise BsedError(f"detect_recording: batch_windows must be at least 1, got {batch_windows}")
    wave, rs, n, mel = _recording_input(wave, sr, resample_quality, mel)
    cfg = mel.cfg
    starts, Tp, T_total = window_plan(n, cfg.sr, cfg.hop_size, pooling_time_ratio, cfg.max_len_seconds, hop_frames)
    classwise_median_window = _learned_windows(learned_post, classwise_median_window, cfg.sr, cfg.hop_size, pooling_time_ratio)
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
            mask = _threshold_mask(stitched[None], t, median_window, learned_post, classwise_median_window)
            return decode_long_gpu(mask[0], scale, duration)
        _, ev_class, _, ev_sec = stage("post", post)
        dfs.append(_event_frame(labels, ev_class, ev_sec, np.full(len(ev_class), filename, dtype=object)))
    predictions = dfs[0] if len(dfs) == 1 else dfs
    return (predictions, stitched, win_probs) if return_probabilities else predictions
