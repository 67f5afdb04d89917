"""Numpy restatement of the reference's clip-level (weak) scoring, TEST INFRASTRUCTURE ONLY: a transcription of
``get_f_measure_by_class`` after the forward (reference src/evaluation_measures.py:386-427) and of
``intermediate_at_measures`` (:442-446), applied to one batch or summed over several.  It shares nothing with the GPU
kernel: whole-array numpy compares, float64 sums.

``ProbabilityEncoder().binarization`` is dcase_util's, which is not installed where this project is developed; SURVEY.md
records it as ``probabilities > threshold``, and that strict compare is what ``binarization`` below states.  How the
library treats ``p == threshold`` is therefore not pinned against it."""
import numpy as np


def binarization(probabilities, threshold):
    """dcase_util ProbabilityEncoder.binarization, 'global_threshold' (a number) and 'class_threshold' with time_axis=0
    (a list with one entry per column): 1.0 where the probability lies above its threshold.  The compare runs in the
    probabilities' own float32, as numpy runs ``float32_array > python_float``."""
    p = np.asarray(probabilities)
    thr = np.asarray(threshold, dtype=p.dtype)          # () or (C): broadcasts over the clip axis
    return (p > thr).astype(np.float64)


def intermediate_at_measures(encoded_ref, encoded_est):
    """reference :442-446, verbatim arithmetic"""
    tp = (encoded_est + encoded_ref == 2).sum(axis=0)
    fp = (encoded_est - encoded_ref == 1).sum(axis=0)
    fn = (encoded_ref - encoded_est == 1).sum(axis=0)
    tn = (encoded_est + encoded_ref == 0).sum(axis=0)
    return tp, fp, fn, tn


def reduce_batch(pred_weak, labels):
    """reference :386-398: what one loader batch is reduced to before any threshold is applied -> ((B,C), (B,C))"""
    pred_weak, labels = np.asarray(pred_weak), np.asarray(labels)
    if len(pred_weak.shape) == 3:                       # :390-392, a model predicting only strong outputs
        pred_weak = np.max(pred_weak, axis=1)
    if len(labels.shape) == 3:                          # :394-398
        labels = np.max(labels, axis=1)
        labels = binarization(labels, 0.5)
    return pred_weak, labels


def batch_counts(pred_weak, labels, thresholds_=None, threshold=0.5):
    """one reduced batch, reference :400-417 -> (tp, fp, fn, tn), each (C)"""
    thresh = threshold if thresholds_ is None else list(thresholds_)     # :400-406
    batch_predictions = binarization(pred_weak, thresh)                 # :408-412
    return intermediate_at_measures(labels, batch_predictions)


def counts_np(batches, thresholds):
    """batches: list of (pred_weak, labels); thresholds: (S) numbers or (S,C) per-class rows -> (S,C,4) int64
    (tp, fp, fn, tn), summed over the batches as :417-421 sums them.  The reduction of a batch does not depend on the
    threshold and is made once."""
    reduced = [reduce_batch(p, l) for p, l in batches]
    rows = []
    for t in thresholds:
        per_class = np.ndim(t) > 0
        total = None
        for pred_weak, labels in reduced:
            c = np.stack(batch_counts(pred_weak, labels, thresholds_=list(t) if per_class else None,
                                      threshold=None if per_class else t), -1).astype(np.int64)
            total = c if total is None else total + c
        rows.append(total)
    return np.stack(rows)


def f_measure_np(counts):
    """reference :423-427 on (C,4) counts -> (C) float64"""
    tp, fp, fn = (np.asarray(counts)[:, k].astype(np.float64) for k in range(3))
    macro_f_score = np.zeros(len(tp))
    mask_f_score = 2 * tp + fp + fn != 0
    macro_f_score[mask_f_score] = 2 * tp[mask_f_score] / (2 * tp + fp + fn)[mask_f_score]
    return macro_f_score


def masks_np(pred_weak, threshold=0.5, class_thresholds=None):
    """reference src/audio_tagging_inference.py:297-309 -> (B) uint64, bit c = class c on"""
    pred_weak = np.asarray(pred_weak)
    if len(pred_weak.shape) == 3:
        pred_weak = np.max(pred_weak, axis=1)
    on = binarization(pred_weak, threshold if class_thresholds is None else list(class_thresholds)) == 1
    out = np.zeros(len(on), np.uint64)
    for c in range(on.shape[1]):
        out |= on[:, c].astype(np.uint64) << np.uint64(c)
    return out


# Hand-worked batch: 4 clips x 3 classes, threshold 0.5.
#   scores                 est          targets        per class (tp, fp, fn, tn)
#   0.9  0.5  0.2          1 0 0        1  1  0
#   0.6  0.7  nan          1 1 0        0  1  1
#   0.1  0.4  0.8          0 0 1       -1 -1 -1        (encode_weak("empty"))
#   0.5000001 0.3 0.51     1 0 1        1  0 -1
# class 0: clips est/ref = 1/1 tp, 1/0 fp, 0/-1 (est - ref == 1) fp, 1/1 tp          -> (2, 2, 0, 0)
# class 1: 0/1 fn (score == threshold is OFF), 1/1 tp, 0/-1 fp, 0/0 tn               -> (1, 1, 1, 1)
# class 2: 0/0 tn, nan -> 0 with ref 1 fn, 1/-1 (est + ref == 0) tn, 1/-1 tn          -> (0, 0, 1, 3)
HAND_SCORES = np.asarray([[0.9, 0.5, 0.2], [0.6, 0.7, np.nan], [0.1, 0.4, 0.8], [0.5000001, 0.3, 0.51]], np.float32)
HAND_TARGETS = np.asarray([[1, 1, 0], [0, 1, 1], [-1, -1, -1], [1, 0, -1]], np.float32)
HAND_COUNTS = [[2, 2, 0, 0], [1, 1, 1, 1], [0, 0, 1, 3]]
# the same batch at the per-class thresholds [0.95, 0.3, 0.8]: est = 0 1 0 / 0 1 0 / 0 1 0 (0.8 == 0.8 is off) / 0 0 0
#   (float32(0.3) > float32(0.3) is off)
# class 0: 0/1 fn, 0/0 tn, 0/-1 fp, 0/1 fn -> (0, 1, 2, 1);  class 1: 1/1 tp, 1/1 tp, 1/-1 tn, 0/0 tn -> (2, 0, 0, 2);
# class 2: 0/0 tn, 0/1 fn, 0/-1 fp, 0/-1 fp -> (0, 2, 1, 1)
HAND_CLASS_THRESHOLDS = [0.95, 0.3, 0.8]
HAND_CLASS_COUNTS = [[0, 1, 2, 1], [2, 0, 0, 2], [0, 2, 1, 1]]
