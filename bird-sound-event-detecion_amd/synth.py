"""Strongly labelled training clips synthesized on the GPU.

The reference makes its ``SYN`` set offline: ``desed`` / ``scaper`` place foreground events on backgrounds, write the
clips to disk, and ``syn_preprocess`` turns them into features clip by clip
(src/synth_data/synth_data_preprocess.py:116-188).  Here the event snippets and the backgrounds live on the device in one
flat array (``SoundBank``); a batch of soundscapes is drawn on the host as a few small tables (``plan_soundscapes`` ->
``SoundscapePlan``), and two launches (csrc/synth.hip) mix the ``(B, n)`` waveforms that
``SEDTrainer.train_step(from_wave=True)`` takes and write their ``(B, T', C)`` strong targets.

  SoundBank            <- scaper's fg_folder / bg_folder (``<fg>/<LABEL>/*.wav``, ``<bg>/**/*.wav``)
  plan_soundscapes     <- desed.SoundscapesGenerator.generate / generate_by_label_occurence + rm_high_polyphony
  SoundscapePlan.annotations <- post_process_txt_labels (the reference's same_event_label_overlap,
                          synth_data_preprocess.py:44-61)
  Synthesizer.write_dataset  <- syn_preprocess (synth_data_preprocess.py:82-114): the offline counterpart

Levels: ``loudness="rms"`` (the default) reads ``ref_db`` and the SNR against each item's plain RMS; ``loudness="lufs"``
reads them, as scaper does, against the item's BS.1770-4 integrated loudness, measured on the device by
``bsed_loudness`` under the rules include/bsed.h states (K-weighting, gated 400 ms blocks, a short snippet tiled to half a
second; the whole item is measured, also where a plan cuts a stretch out of it).  NOT pinned to the reference's tools:
scaper's (pyloudnorm's) values were not compared against, and the sampler's draws are this project's own (a numpy
``Generator``), not desed's.  Clips made here have the reference's structure and annotation format, not its sample values
-- as ``features.load_audio`` says about librosa's resampler.
"""
import glob
import os

import numpy as np
import torch

from . import _lib as L
from . import ops, parallel

MAX_EVENTS = L.CONSTANTS["BSED_SYNTH_MAX_EVENTS"]


def frames_of(seconds, sr, hop_size=255, pooling_time_ratio=4):
    """``ManyHotEncoder.frame`` for an array of times: ``int(t * sr // hop // pooling)`` in float64 floor division.
    (NOT ``sample // (hop * pooling)``: the float64 product t * sr can fall below the integer it stands for.)"""
    t = np.asarray(seconds, dtype=np.float64) * sr
    return np.floor_divide(np.floor_divide(t, hop_size), pooling_time_ratio).astype(np.int32)


class SoundBank:
    """Event snippets and backgrounds as ONE flat float32 device array, with host tables of where each item lies.

    events: iterable of ``(label, waveform)``; backgrounds: iterable of waveforms; each waveform 1-D int16 or float32,
    a numpy array or a GPU tensor, already at ``sr`` (int16 is scaled by 1 / 32768 on the device).  Items keep the
    order they are given in: events first, then backgrounds.

      bank.flat                    (total samples,) float32 device tensor
      bank.offset / .length        int64 per item, in samples
      bank.cls                     int32 per item: index into ``labels``, -1 for a background
      bank.rms                     float64 per item (computed once, on the device, in float64)
      bank.lufs                    float64 per item with ``loudness="lufs"`` (-inf: no block above -70 LUFS), else None:
                                   all items measured by ONE ``bsed_loudness`` call over ``flat``
      bank.items(label)            item indices of a label's snippets;  bank.backgrounds: those of the backgrounds
    """

    def __init__(self, events, backgrounds, labels, sr=32000, loudness="rms"):
        from .features import resampler
        if loudness not in ("rms", "lufs"):
            raise L.BsedError(f'SoundBank: loudness must be "rms" or "lufs", got {loudness!r}')
        L._require_gpu()
        self.labels, self.sr = list(labels), int(sr)
        to_f32 = resampler(self.sr, self.sr)          # the convert-only case: int16 -> float32 in one launch
        waves, cls = [], []
        for label, w in events:
            if label not in self.labels:
                raise L.BsedError(f"SoundBank: label {label!r} is not one of the {len(self.labels)} labels")
            waves.append(w)
            cls.append(self.labels.index(label))
        n_events = len(waves)
        for w in backgrounds:
            waves.append(w)
            cls.append(-1)
        if not waves:
            raise L.BsedError("SoundBank: no snippets and no backgrounds")
        dev = []
        for k, w in enumerate(waves):
            what = f"snippet {k} ({self.labels[cls[k]]})" if k < n_events else f"background {k - n_events}"
            if not isinstance(w, (np.ndarray, torch.Tensor)) or w.ndim != 1:
                raise L.BsedError(f"SoundBank: {what} must be a 1-D numpy array or GPU tensor")
            if int(w.shape[0]) < 1:
                raise L.BsedError(f"SoundBank: {what} is empty")
            dev.append(to_f32(w))
        self.flat = torch.cat(dev).contiguous()
        length = [int(w.shape[0]) for w in dev]
        levels = torch.stack([w.double().pow(2).mean().sqrt() for w in dev])
        if loudness == "lufs":
            ln = torch.tensor(length, dtype=torch.int64)
            off = torch.cumsum(ln, 0) - ln
            lufs = ops.loudness(self.flat, off.to(self.flat.device), ln.to(self.flat.device), self.sr, max(length),
                                samples=sum(length))
            levels = torch.cat([levels, lufs])
        levels = levels.cpu().numpy()                                                             # the one host sync
        self._set_tables(length, cls, levels[:len(dev)], levels[len(dev):] if loudness == "lufs" else None)

    def _set_tables(self, length, cls, rms, lufs=None):
        self.length = np.asarray(length, dtype=np.int64).reshape(-1)
        self.cls = np.asarray(cls, dtype=np.int32).reshape(-1)
        self.rms = np.asarray(rms, dtype=np.float64).reshape(-1)
        if not len(self.length) == len(self.cls) == len(self.rms) or len(self.length) < 1:
            raise L.BsedError("SoundBank: one length, class and RMS per item, and at least one item")
        self.lufs = None if lufs is None else np.asarray(lufs, dtype=np.float64).reshape(-1)
        if self.lufs is not None and (len(self.lufs) != len(self.length) or np.isnan(self.lufs).any() or
                                      np.isposinf(self.lufs).any()):
            raise L.BsedError("SoundBank: one loudness per item, each a number or -inf")
        if (self.length < 1).any() or (self.cls >= len(self.labels)).any():
            raise L.BsedError("SoundBank: an empty item or a class outside the labels")
        self.offset = np.concatenate([[0], np.cumsum(self.length)[:-1]]).astype(np.int64)
        self.backgrounds = np.nonzero(self.cls < 0)[0]
        self._by_class = [np.nonzero(self.cls == c)[0] for c in range(len(self.labels))]

    @classmethod
    def layout(cls, labels, length, item_class, rms, sr=32000, lufs=None):
        """A bank described by its host tables alone (``flat`` is None): enough to draw and validate plans -- which is
        host work -- on a machine without the samples or without a GPU.  item_class: label index, -1 = background;
        lufs: the items' integrated loudness, for plans drawn with ``loudness="lufs"``."""
        self = cls.__new__(cls)
        self.labels, self.sr, self.flat = list(labels), int(sr), None
        self._set_tables(length, item_class, rms, lufs)
        return self

    def __len__(self):
        return len(self.length)

    @property
    def total_samples(self):
        return int(self.length.sum())

    def items(self, label):
        if label not in self.labels:
            raise L.BsedError(f"SoundBank.items: unknown label {label!r}")
        return self._by_class[self.labels.index(label)]

    def wave(self, item):
        """the samples of one item (a view of ``flat``)"""
        return self.flat[int(self.offset[item]):int(self.offset[item] + self.length[item])]

    @classmethod
    def from_folders(cls, fg_folder, bg_folder, labels, sr=32000, loudness="rms"):
        """scaper's layout: ``<fg_folder>/<LABEL>/*.wav`` and ``<bg_folder>/**/*.wav`` (``bg_folder`` may be None).  Files
        are read with ``features.load_audio``: any rate and channel count, mixed to mono and resampled to ``sr`` on the
        GPU.  Files are taken in sorted order, so the bank does not depend on the directory's listing order.
        ``loudness`` is the bank's."""
        from .features import load_audio
        labels = list(labels)
        events = []
        for d in sorted(os.listdir(fg_folder)):
            if not os.path.isdir(os.path.join(fg_folder, d)):
                continue
            if d not in labels:
                raise L.BsedError(f"SoundBank.from_folders: {os.path.join(fg_folder, d)}: {d!r} is not one of the labels")
            for path in sorted(glob.glob(os.path.join(fg_folder, d, "*.wav"))):
                events.append((d, load_audio(path, sr)[0]))
        bgs = []
        if bg_folder is not None:
            for path in sorted(glob.glob(os.path.join(bg_folder, "**", "*.wav"), recursive=True)):
                bgs.append(load_audio(path, sr)[0])
        return cls(events, bgs, labels, sr, loudness)


class SoundscapePlan:
    """The host tables of one batch of soundscapes: exactly the inputs of ``bsed_synth_mix`` and ``bsed_synth_targets``
    (include/bsed.h), as numpy arrays.

      per clip (B):      bg_off, bg_len, bg_phase int64; bg_gain float32; n_ev int32
      per event (B, K):  src, on, len int64; g, inv_fade float32; cls int32   (slots k >= n_ev[b] are unused)
      derived (B, K):    onset_s = on / sr, offset_s = (on + len) / sr  float64;
                         on_f, off_f int32 = the encoder's frames of those seconds (``frames_of``)

    A plan may be built by hand from arrays; ``validate(bank)`` is what stands between a plan and the device."""

    def __init__(self, n, sr, labels, bg_off, bg_len, bg_phase, bg_gain, n_ev, src, on, length, g, inv_fade, cls,
                 hop_size=255, pooling_time_ratio=4, names=None):
        self.n, self.sr, self.labels = int(n), int(sr), list(labels)
        self.hop_size, self.pooling_time_ratio = hop_size, pooling_time_ratio
        self.n_ev = np.ascontiguousarray(n_ev, dtype=np.int32).reshape(-1)
        self.B = len(self.n_ev)
        per_clip = lambda a, dt: np.ascontiguousarray(a, dtype=dt).reshape(self.B)
        self.bg_off, self.bg_len, self.bg_phase = (per_clip(a, np.int64) for a in (bg_off, bg_len, bg_phase))
        self.bg_gain = per_clip(bg_gain, np.float32)
        self.src = np.ascontiguousarray(src, dtype=np.int64).reshape(self.B, -1)
        self.K = self.src.shape[1]
        per_event = lambda a, dt: np.ascontiguousarray(a, dtype=dt).reshape(self.B, self.K)
        self.on, self.len = per_event(on, np.int64), per_event(length, np.int64)
        self.g, self.inv_fade = per_event(g, np.float32), per_event(inv_fade, np.float32)
        self.cls = per_event(cls, np.int32)
        self.names = [f"{b}" for b in range(self.B)] if names is None else list(names)
        self.onset_s = self.on.astype(np.float64) / self.sr
        self.offset_s = (self.on + self.len).astype(np.float64) / self.sr
        self.on_f = frames_of(self.onset_s, self.sr, hop_size, pooling_time_ratio)
        self.off_f = frames_of(self.offset_s, self.sr, hop_size, pooling_time_ratio)

    @property
    def used(self):
        """(B, K) bool: the slots that hold an event"""
        return np.arange(self.K)[None, :] < self.n_ev[:, None]

    @property
    def coverage(self):
        """mean number of events over an output sample"""
        return float((self.len * self.used).sum()) / (self.B * self.n)

    def validate(self, bank):
        """Raise ``BsedError`` unless every table entry the kernels will read is inside the clip and inside ONE item of
        the bank.  (The kernel itself only promises not to read outside the bank.)"""
        def bad(msg):
            raise L.BsedError("SoundscapePlan: " + msg)
        if self.K > MAX_EVENTS:
            bad(f"K = {self.K} exceeds BSED_SYNTH_MAX_EVENTS = {MAX_EVENTS}")
        if self.sr != bank.sr:
            bad(f"plan at {self.sr} Hz, bank at {bank.sr} Hz")
        if self.n < 1:
            bad(f"n = {self.n}")
        if ((self.n_ev < 0) | (self.n_ev > self.K)).any():
            bad(f"n_ev outside 0..K = {self.K}: {self.n_ev[(self.n_ev < 0) | (self.n_ev > self.K)][:4].tolist()}")
        ends = bank.offset + bank.length

        def inside_one_item(off, length):
            item = np.searchsorted(bank.offset, off, side="right") - 1
            return (off >= 0) & (item >= 0) & (off + length <= ends[np.clip(item, 0, len(ends) - 1)])
        u = self.used
        b_of = np.nonzero(u)[0]
        on, ln, src, g, f, c = (a[u] for a in (self.on, self.len, self.src, self.g, self.inv_fade, self.cls))
        for cond, msg in (
                (ln < 1, "an event with len < 1"),
                ((on < 0) | (on + ln > self.n), "an event that leaves the clip"),
                (~inside_one_item(src, np.maximum(ln, 1)), "an event that leaves its snippet"),
                (~(g >= 0) | ~np.isfinite(g), "a negative or non-finite gain"),
                (~((f > 0) & (f <= 1)), "inv_fade outside (0, 1]"),
                ((c < 0) | (c >= len(self.labels)), "a class outside the labels")):
            if cond.any():
                k = int(np.nonzero(cond)[0][0])
                bad(f"{msg} (clip {int(b_of[k])}: on={int(on[k])}, len={int(ln[k])}, src={int(src[k])}, g={float(g[k])}, "
                    f"inv_fade={float(f[k])}, class={int(c[k])}; n={self.n})")
        if (self.bg_len < 0).any():
            bad("a negative bg_len")
        has = self.bg_len > 0
        if (~inside_one_item(self.bg_off[has], self.bg_len[has])).any():
            bad("a background that leaves its bank item")
        if (self.bg_phase[has] < 0).any():
            bad("a negative bg_phase")
        if (~(self.bg_gain >= 0) | ~np.isfinite(self.bg_gain)).any():
            bad("a negative or non-finite bg_gain")
        return self

    def events(self, b):
        """[(onset_s, offset_s, label), ...] of clip b, in table order"""
        return [(float(self.onset_s[b, k]), float(self.offset_s[b, k]), self.labels[self.cls[b, k]])
                for k in range(int(self.n_ev[b]))]

    def annotations(self, merge_same_label=True):
        """DataFrame ``filename / onset / offset / event_label`` (seconds), clip by clip.  merge_same_label: events of one
        label that overlap or touch become one row from the first onset to the last offset, as the reference's
        ``post_process_txt_labels`` leaves them (a row starts a new group when its onset lies beyond every earlier
        offset of its label); events of different labels are never joined."""
        import pandas as pd
        rows = []
        for b in range(self.B):
            ev = self.events(b)
            if merge_same_label:
                merged = []
                for label in sorted({e[2] for e in ev}):
                    cur = None
                    for on, off, _ in sorted(e for e in ev if e[2] == label):
                        if cur is not None and on <= cur[1]:
                            cur[1] = max(cur[1], off)
                        else:
                            cur = [on, off, label]
                            merged.append(cur)
                ev = sorted(map(tuple, merged))
            rows += [(self.names[b] + ".wav", on, off, label) for on, off, label in ev]
        return pd.DataFrame(rows, columns=["filename", "onset", "offset", "event_label"])


def _polyphony_with(intervals, on, off):
    """the largest number of simultaneously active events inside [on, off) once that interval joins ``intervals``"""
    worst = 0
    for p in [on] + [a for a, _ in intervals if on < a < off]:
        worst = max(worst, sum(1 for a, z in intervals if a <= p < z))
    return worst + 1


def plan_soundscapes(bank, B, rng, clip_seconds=10.0, n_events=(1, 6), class_probs=None, co_occurrence=None,
                     snr_db=(6.0, 30.0), ref_db=-55.0, max_polyphony=4, min_event_seconds=0.2, fade_seconds=0.01,
                     n_samples=None, hop_size=255, pooling_time_ratio=4, max_events=MAX_EVENTS, names=None, loudness="rms"):
    """Draw B soundscapes over ``bank`` on the host -> ``SoundscapePlan``.  ``rng`` is a ``numpy.random.Generator``; no
    global state is read and the same generator state gives the same plan.

    Events of a clip: ``n_events`` = (lo, hi), uniform and inclusive, with classes drawn by ``class_probs`` (one weight per
    label; None: uniform over the labels that have snippets).  With ``co_occurrence`` -- a dict in the format of the
    reference's ``event_occurences*.json``: per main class ``proba`` and ``co-occurences.{max_events, mean_events, classes,
    probas}`` -- the main class is drawn by ``proba``, one event of it is placed, then
    ``min(max_events, Poisson(mean_events)) - 1`` further events with classes drawn by ``probas``.  Never more than
    ``max_events`` (at most BSED_SYNTH_MAX_EVENTS) per clip.

    Placement: a snippet of the class is drawn uniformly and used whole; one longer than the clip is cut to a random
    n-sample stretch.  ``min_event_seconds`` is the shortest stretch a snippet may be cut to (a clip shorter than it is
    refused); shorter snippets are used as they are.  The onset is uniform over [0, n - len].  A draw that would take the
    number of simultaneously active events above ``max_polyphony`` (the reference's ``rm_high_polyphony``) is redrawn up
    to 20 times, then dropped.  ``fade_seconds``: linear fade-in and fade-out of every event.

    Levels, with ``snr`` uniform over ``snr_db`` and ``ref_db = -55`` the reference's (src/synth_data/data_config.py:5):
    ``loudness="rms"``: ``bg_gain = 10^(ref_db / 20) / rms(background)`` and ``g = 10^((ref_db + snr) / 20) / rms(snippet)``;
    ``loudness="lufs"`` (scaper's reading of the two numbers; the bank must carry ``lufs``):
    ``bg_gain = 10^((ref_db - lufs(background)) / 20)`` and ``g = 10^((ref_db + snr - lufs(snippet)) / 20)``, formed in
    float64 and rounded to float32.  ``lufs`` is ``bsed_loudness``'s value of the WHOLE item (include/bsed.h), so a
    background alone in a clip measures ``ref_db`` and an event ``ref_db + snr`` when it is placed whole; scaper's own
    values are not pinned.  A silent item (RMS 0, or -inf LUFS) gets gain 0.  The draws do not depend on ``loudness``: the
    two plans of one generator state differ in ``g`` and ``bg_gain`` alone.  Without backgrounds in the bank every clip has
    ``bg_len = 0`` (silence under the events).

    ``n_samples`` overrides ``clip_seconds * sr``; ``hop_size`` / ``pooling_time_ratio`` are the encoder's, for the
    frame tables."""
    if not isinstance(rng, np.random.Generator):
        raise L.BsedError("plan_soundscapes: rng must be a numpy.random.Generator")
    sr = bank.sr
    n = int(n_samples) if n_samples is not None else int(round(clip_seconds * sr))
    K = int(max_events)
    if not 1 <= K <= MAX_EVENTS:
        raise L.BsedError(f"plan_soundscapes: max_events must be in 1..{MAX_EVENTS}, got {max_events}")
    min_len = int(np.ceil(min_event_seconds * sr))
    if n < max(min_len, 1):
        raise L.BsedError(f"plan_soundscapes: a clip of {n} samples is shorter than min_event_seconds = {min_event_seconds}")
    if B < 1 or max_polyphony < 1:
        raise L.BsedError("plan_soundscapes: B and max_polyphony must be at least 1")
    if loudness not in ("rms", "lufs"):
        raise L.BsedError(f'plan_soundscapes: loudness must be "rms" or "lufs", got {loudness!r}')
    if loudness == "lufs" and getattr(bank, "lufs", None) is None:
        raise L.BsedError('plan_soundscapes: loudness="lufs" needs a bank that carries lufs (SoundBank(..., loudness="lufs"))')
    C = len(bank.labels)
    have = np.array([len(bank._by_class[c]) > 0 for c in range(C)])
    if co_occurrence is None:
        lo, hi = int(n_events[0]), int(n_events[1])
        if not 0 <= lo <= hi:
            raise L.BsedError(f"plan_soundscapes: n_events must be (lo, hi) with 0 <= lo <= hi, got {n_events}")
        p = have.astype(np.float64) if class_probs is None else np.asarray(class_probs, dtype=np.float64)
        if p.shape != (C,) or (p < 0).any() or (p[~have] > 0).any() or (hi > 0 and p.sum() <= 0):
            raise L.BsedError("plan_soundscapes: class_probs must hold one non-negative weight per label, zero for labels "
                              "without snippets, and not all zero")
        p = p / p.sum() if p.sum() > 0 else p
    else:
        mains = list(co_occurrence)
        for m in mains:
            for lab in [m] + list(co_occurrence[m]["co-occurences"]["classes"]):
                if lab not in bank.labels or not have[bank.labels.index(lab)]:
                    raise L.BsedError(f"plan_soundscapes: co_occurrence names {lab!r}, which has no snippet in the bank")
        p_main = np.array([float(co_occurrence[m]["proba"]) for m in mains])
        p_main = p_main / p_main.sum()
    fade = max(1, int(round(fade_seconds * sr)))
    inv_fade_v = np.float32(1.0 / fade)
    ref_amp = 10.0 ** (ref_db / 20.0)

    # every draw of the batch is made in bulk, in a fixed sequence (the plan of a generator state depends on B); the only
    # per-event host work left is the polyphony test
    P = dict(bg_off=np.zeros(B, np.int64), bg_len=np.zeros(B, np.int64), bg_phase=np.zeros(B, np.int64),
             bg_gain=np.zeros(B, np.float32), n_ev=np.zeros(B, np.int32), src=np.zeros((B, K), np.int64),
             on=np.zeros((B, K), np.int64), length=np.ones((B, K), np.int64), g=np.zeros((B, K), np.float32),
             inv_fade=np.full((B, K), inv_fade_v, np.float32), cls=np.zeros((B, K), np.int32))
    safe_rms = np.where(bank.rms > 0, bank.rms, np.inf)          # a silent item: gain 0

    def lufs_gain(items, level_db):
        """float32 gains that bring the items' integrated loudness to level_db (a scalar, or one level per item)"""
        lufs = bank.lufs[items]
        quiet = np.isneginf(lufs)                                # a silent item: gain 0
        return np.where(quiet, 0.0, 10.0 ** ((level_db - np.where(quiet, 0.0, lufs)) / 20.0)).astype(np.float32)
    if len(bank.backgrounds):
        it = bank.backgrounds[rng.integers(len(bank.backgrounds), size=B)]
        P["bg_off"], P["bg_len"] = bank.offset[it], bank.length[it]
        P["bg_phase"] = np.minimum((rng.random(B) * bank.length[it]).astype(np.int64), bank.length[it] - 1)
        P["bg_gain"] = lufs_gain(it, ref_db) if loudness == "lufs" else (ref_amp / safe_rms[it]).astype(np.float32)
    if co_occurrence is None:
        count = np.minimum(rng.integers(lo, hi + 1, size=B), K)
        classes = rng.choice(C, size=int(count.sum()), p=p) if count.sum() else np.zeros(0, np.int64)
    else:
        main = rng.choice(len(mains), size=B, p=p_main)
        cos = [co_occurrence[m]["co-occurences"] for m in mains]
        drawn = rng.poisson(np.array([float(co["mean_events"]) for co in cos])[main])
        count = np.clip(np.minimum(drawn, np.array([int(co["max_events"]) for co in cos])[main]), 1, K)
        first = np.concatenate([[0], np.cumsum(count)[:-1]])
        classes = np.zeros(int(count.sum()), np.int64)
        classes[first] = np.array([bank.labels.index(m) for m in mains])[main]
        for mi, co in enumerate(cos):                            # the further events of the clips of one main class
            slots = np.concatenate([np.arange(first[b] + 1, first[b] + count[b]) for b in np.nonzero(main == mi)[0]] or
                                   [np.zeros(0, np.int64)]).astype(np.int64)
            pc = np.asarray(co["probas"], dtype=np.float64)
            ids = np.array([bank.labels.index(c) for c in co["classes"]])
            classes[slots] = ids[rng.choice(len(ids), size=len(slots), p=pc / pc.sum())]
    E = len(classes)
    clip = np.repeat(np.arange(B), count)
    u_item, u_start, u_on = rng.random(E), rng.random(E), rng.random((E, 21))      # 21: the draw and up to 20 redraws
    snr = rng.uniform(snr_db[0], snr_db[1], size=E)
    n_items = np.array([len(x) for x in bank._by_class])
    pick = np.minimum((u_item * n_items[classes]).astype(np.int64), n_items[classes] - 1)
    item = np.array([bank._by_class[c][k] for c, k in zip(classes.tolist(), pick.tolist())], dtype=np.int64)
    full = bank.length[item] if E else np.zeros(0, np.int64)
    length = np.minimum(full, n)
    start = np.minimum((u_start * (full - length + 1)).astype(np.int64), full - length)
    room = (n - length + 1)[:, None]
    onsets = np.minimum((u_on * room).astype(np.int64), room - 1)
    if not E:
        gain = np.zeros(0, np.float32)
    elif loudness == "lufs":
        gain = lufs_gain(item, ref_db + snr)
    else:
        gain = (ref_amp * 10.0 ** (snr / 20.0) / safe_rms[item]).astype(np.float32)
    keep_on = np.full(E, -1, np.int64)
    slot = np.zeros(E, np.int64)
    placed, cur = [], -1
    for e, (b, ln, cand) in enumerate(zip(clip.tolist(), length.tolist(), onsets.tolist())):
        if b != cur:
            placed, cur = [], b
        for on in cand:
            # fewer than max_polyphony events in the clip cannot be too many anywhere
            if len(placed) < max_polyphony or _polyphony_with(placed, on, on + ln) <= max_polyphony:
                keep_on[e], slot[e] = on, len(placed)
                placed.append((on, on + ln))
                break
    kept = keep_on >= 0                                          # the others ran out of redraws: dropped
    bk = (clip[kept], slot[kept])
    P["src"][bk], P["on"][bk], P["length"][bk] = (bank.offset[item] + start)[kept], keep_on[kept], length[kept]
    P["cls"][bk], P["g"][bk] = classes[kept], gain[kept]
    P["n_ev"] = np.bincount(clip[kept], minlength=B).astype(np.int32)
    return SoundscapePlan(n, sr, bank.labels, hop_size=hop_size, pooling_time_ratio=pooling_time_ratio, names=names, **P)


class PlanTables:
    """A plan's tables on the device: ONE pinned host buffer, one non-blocking copy, views of the device buffer."""
    _I64 = ("bg_off", "bg_len", "bg_phase", "src", "on", "len")
    _F32 = ("bg_gain", "g", "inv_fade")
    _I32 = ("n_ev", "cls", "on_f", "off_f")

    def __init__(self, plan, device):
        parts, pos = [], 0
        for names, width, tdt in ((self._I64, 8, torch.int64), (self._F32, 4, torch.float32), (self._I32, 4, torch.int32)):
            for name in names:
                a = getattr(plan, name)
                parts.append((name, a, pos, tdt))
                pos += (a.size * width + 15) // 16 * 16
        host = torch.empty(max(pos, 16), dtype=torch.uint8, pin_memory=True)
        view = host.numpy()
        for name, a, at, _ in parts:
            view[at:at + a.nbytes] = a.reshape(-1).view(np.uint8)
        # the pinned block returns to torch's host allocator only after the copy has run on this stream
        self.buffer = host.to(device, non_blocking=True)
        for name, a, at, tdt in parts:
            setattr(self, name, self.buffer[at:at + a.nbytes].view(tdt).view(a.shape))


def mix(bank, plan, tables=None, K=None, out=None):
    """The (B, n) waveforms of a VALIDATED plan (``plan.validate(bank)``).  K: how many event slots per clip the kernel is
    given (default: all of the plan's; any K >= max n_ev gives the same bits)."""
    t = tables or PlanTables(plan, bank.flat.device)
    K = plan.K if K is None else int(K)
    if K == plan.K:
        ev = [t.src, t.on, t.len, t.g, t.inv_fade]
    else:
        if not int(plan.n_ev.max(initial=0)) <= K <= plan.K:
            raise L.BsedError(f"synth.mix: K = {K} must lie between the largest n_ev and the plan's K = {plan.K}")
        ev = [a[:, :K].contiguous() for a in (t.src, t.on, t.len, t.g, t.inv_fade)]
    return ops.synth_mix(bank.flat, t.bg_off, t.bg_len, t.bg_phase, t.bg_gain, t.n_ev, *ev, plan.B, plan.n, K,
                         coverage=plan.coverage if L.timer is not None else 0.0, out=out)


def targets(plan, n_frames, tables=None, device=None):
    """(strong (B, n_frames, C), weak (B, C)) of a plan, written by one launch"""
    t = tables or PlanTables(plan, device or "cuda")
    return ops.synth_targets(t.n_ev, t.cls, t.on_f, t.off_f, plan.B, plan.K, int(n_frames), len(plan.labels))


class Synthesizer:
    """Batches of synthetic strongly labelled clips for ``SEDTrainer.train_step(from_wave=True)``.

    encoder: a ``labels.ManyHotEncoder`` -- its labels (which must be the bank's), ``n_frames``, rate, hop and pooling
    define the targets.  ``plan_kw`` goes to ``plan_soundscapes``.  The generator of a batch is seeded by
    ``parallel.rank_seed(seed, step, rank)``: the batch of a step repeats across runs and differs across ranks.

        w0, y0, *_ = synth.batch(B, 0)
        for k in range(steps):
            w1, y1, *_ = synth.batch(B, k + 1)
            trainer.train_step(w0, y0, from_wave=True, next_waves=(w1, None))
            w0, y0 = w1, y1
    """

    def __init__(self, bank, encoder, n_samples, seed=2023, rank=None, **plan_kw):
        if list(encoder.labels) != list(bank.labels):
            raise L.BsedError("Synthesizer: the encoder's labels are not the bank's")
        if encoder.sr != bank.sr:
            raise L.BsedError(f"Synthesizer: encoder at {encoder.sr} Hz, bank at {bank.sr} Hz")
        if not encoder.n_frames or encoder.n_frames < 1:
            raise L.BsedError("Synthesizer: the encoder needs n_frames")
        self.bank, self.encoder, self.n_samples, self.seed = bank, encoder, int(n_samples), seed
        if rank is None:
            dist = torch.distributed
            rank = dist.get_rank() if dist.is_available() and dist.is_initialized() else 0
        self.rank = int(rank)
        self.plan_kw = dict(plan_kw, n_samples=self.n_samples, hop_size=encoder.hop_size,
                            pooling_time_ratio=encoder.pooling_time_ratio)

    def plan(self, B, step, names=None):
        rng = np.random.default_rng(parallel.rank_seed(self.seed, step, self.rank))
        return plan_soundscapes(self.bank, B, rng, names=names, **self.plan_kw).validate(self.bank)

    def batch(self, B, step, names=None):
        """-> (waves (B, n) float32, strong (B, T', C) float32, weak (B, C) float32, plan): device tensors made by two
        launches behind one table upload on the current stream; nothing waits for the device."""
        plan = self.plan(B, step, names)
        tables = PlanTables(plan, self.bank.flat.device)
        waves = mix(self.bank, plan, tables)
        strong, weak = targets(plan, self.encoder.n_frames, tables)
        return waves, strong, weak, plan

    def batches(self, B, steps, first_step=0):
        for step in range(first_step, first_step + steps):
            yield self.batch(B, step)

    def write_dataset(self, out_dir, n_clips, B=64, frontend=None):
        """The offline counterpart of the reference's ``syn_preprocess``: ``<out_dir>/wav/<name>.npy`` (linear mel of the
        clip, ``MelFrontEnd.linear`` on the batch) and ``<out_dir>/annotation/<name>.txt`` (TSV onset / offset /
        event_label, same-label overlaps merged) for ``n_clips`` clips named ``syn_00000`` ...; batch k of the run is
        ``batch(B, k)``.  ``data.FeatureDataset`` reads the result.  Returns the names."""
        from .features import MelConfig, MelFrontEnd
        fe = frontend or MelFrontEnd(MelConfig(sr=self.bank.sr, hop_size=self.encoder.hop_size))
        os.makedirs(os.path.join(out_dir, "wav"), exist_ok=True)
        os.makedirs(os.path.join(out_dir, "annotation"), exist_ok=True)
        done, step, all_names = 0, 0, []
        while done < n_clips:
            nb = min(B, n_clips - done)
            names = [f"syn_{done + i:05d}" for i in range(nb)]
            waves, _, _, plan = self.batch(nb, step, names)
            mel = fe.linear(waves)[0].cpu().numpy()
            ann = plan.annotations(merge_same_label=True)
            for i, name in enumerate(names):
                np.save(os.path.join(out_dir, "wav", name + ".npy"), mel[i])
                rows = ann[ann["filename"] == name + ".wav"].drop(columns=["filename"])
                rows.to_csv(os.path.join(out_dir, "annotation", name + ".txt"), sep="\t", index=False)
            all_names += names
            done, step = done + nb, step + 1
        return all_names
