"""Clip-level tagging: the reference's per-class weak F1 (src/evaluation_measures.py:346-446, the number ``baseline_best``
is kept by in src/pseudo_labeling_main.py:990-1035) with the tp / fp / fn / tn of a whole threshold sweep counted on the
GPU (``tag_counts_gpu``, one launch per batch, read once per pass), and the pseudo weak labels of an unlabelled pool
(src/audio_tagging_inference.py:289-316) as one bit mask per clip (``bsed_tag_masks``), written as the
``filename<TAB>event_labels`` TSV that ``data.PseudoWeakDataset`` reads."""
from fractions import Fraction

import numpy as np
import torch

from .. import _lib as L
from .._lib import BsedError
from ._common import (_accumulator, _batches, _check_form, _eval_mode, _forward, _host_counts, _required_labels,
                      _write_tsv)

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
    out = _accumulator(out, (thr.S, C, 4), x.device, "tag_counts_gpu")
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
    c = _host_counts(counts, 4, "tag_f1 takes (..., C, 4) counts").astype(np.float64)
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
    labels = _required_labels(decoder, "decode_weak", "pseudo_label", "thresholds")
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
        _write_tsv(df, save_path)
    return df
