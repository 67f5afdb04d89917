"""What every evaluation pass shares: the eval-mode forward of the loader passes, the annotation files, the prediction
frame, the two launches of a decoder, and the small host steps of the scorers (counts to numpy, accumulators, the macro
average, the label list of a decoder, writing a TSV)."""
import os
from contextlib import contextmanager as _contextmanager

import numpy as np
import torch

from .. import _lib as L
from .._lib import BsedError


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


def _required_labels(decoder, method_name, who, why):
    """``_encoder_labels`` for the passes that cannot do without: ``who`` ``why`` (what it does) on the GPU"""
    labels = _encoder_labels(decoder, method_name)
    if labels is None:
        raise BsedError(f"{who} {why} on the GPU and needs the label list: pass the bound {method_name} of a "
                        "ManyHotEncoder as decoder")
    return labels


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


def _write_tsv(df, path, **kw):
    """``df`` as a tab-separated file without the index; the folder of ``path`` is made if it is missing"""
    if os.path.dirname(path):
        os.makedirs(os.path.dirname(path), exist_ok=True)
    df.to_csv(path, index=False, sep="\t", **kw)


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


def _accumulator(out, shape, device, who, must_be=None):
    """the int64 accumulator of a counting call: zeros of ``shape`` when ``out`` is None, else ``out`` after its shape
    check (``must_be``: the caller's own wording of what it takes, when ``out`` is more than this one tensor)"""
    if out is None:
        return torch.zeros(shape, device=device, dtype=torch.int64)
    if tuple(out.shape) != tuple(shape):
        raise BsedError(f"{who}: out must be " + (must_be or f"{tuple(shape)}, got {tuple(out.shape)}"))
    return out


def _host_counts(a, last, who):
    """(..., C, ``last``) counts, GPU tensor or array -> numpy; ``who``: the caller's sentence about what it takes"""
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    if a.ndim < 2 or a.shape[-1] != last:
        raise BsedError(f"{who}, got shape {a.shape}")
    return a


def _macro_in_class_order(class_f1):
    """(..., C) per-class F -> (...) mean over the classes whose F is not NaN, NaN if there is none"""
    valid = ~np.isnan(class_f1)
    n_valid = valid.sum(-1)
    total = np.zeros(n_valid.shape)
    for k in range(class_f1.shape[-1]):                 # summed in class order, so that the value is defined to the bit
        total = total + np.where(valid[..., k], class_f1[..., k], 0.0)
    return np.divide(total, n_valid, out=np.full(n_valid.shape, np.nan), where=n_valid > 0)
