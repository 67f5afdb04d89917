"""Dataset scaler -- the reference's ``Scaler`` (src/utilities/Scaler.py:13-135) with its statistics made on the GPU.

The reference's mean-teacher and adversarial drivers build a ``Scaler``, run ``calculate_scaler`` over the training sets,
hand it to ``get_transforms`` (``Normalize(scaler)`` is the last transform, after ApplyLog / PadOrTrunc / ToTensor, on
both members of the (clean, noisy) pair) and write it into every checkpoint.  Here:

  statistics     ``update`` / ``update_db`` / ``update_waves`` add a batch's per-band sums of x and x^2 to a (2, n_mels)
                 float64 accumulator on the GPU (csrc/scaler.hip): from LINEAR mel the dB value is made on the fly, one
                 read of the mel and no dB tensor.  No host sync until ``finish()`` reads the accumulator once.
  normalisation  ``MelFrontEnd(cfg, scaler)`` / ``MelFrontEnd.set_scaler`` folds ``normalize`` into the dB kernels'
                 epilogue; ``Scaler.normalize`` itself launches a kernel for a GPU tensor and is numpy for numpy arrays
                 and CPU tensors (import-swapped scripts and CPU tests need no GPU).
  persistence    the reference's JSON and state dict: two lists, ``mean_`` and ``mean_of_square_``; ``std_`` is derived.

Arithmetic contract: x^2 is a float32 product widened to float64 (the reference squares a float32 array), the sums are
float64; with equal clip shapes the reference's mean of per-clip means is the global mean up to rounding.  An element is
normalised as ``float32((float64(x) - mean_[m]) / std_[m])``: numpy's promotion followed by ``torch.Tensor(...)``'s cast.
``ScalerPerAudio`` is not provided (every reference driver has it commented out).
"""
import json

import numpy as np
import torch

from . import _lib as L
from . import ops


def _bad_bands(mean, mean_of_square):
    """std_ = sqrt(mean_of_square_ - mean_**2) and the bands it cannot normalise (std_ zero, nan, inf, or a negative
    variance); the reference would feed the model inf or nan there"""
    with np.errstate(invalid="ignore"):
        std = np.sqrt(mean_of_square - mean ** 2)
    bad = np.flatnonzero(~(np.isfinite(std) & (std > 0) & np.isfinite(mean)))
    return std, bad


class Scaler:
    """operates on one or multiple existing datasets and normalises batches with their per-band statistics"""

    def __init__(self):
        self.mean_ = None
        self.mean_of_square_ = None
        self.std_ = None
        self._acc = None          # (2, n_mels) float64 on the GPU: sum of x, sum of x^2
        self._frames = 0          # frames behind _acc (clips * frames per clip)
        self._shape = None        # (frames per clip, n_mels) of every update
        self._dev = {}            # device -> (mean, std) float64 vectors

    # ---- statistics -------------------------------------------------------------------------------------------------
    def _begin(self, who, B, T_out, M, device):
        """host-side checks of one update, before any launch; makes the accumulator on first use"""
        if not 1 <= M <= 256:
            raise L.BsedError(f"Scaler.{who}: n_mels must be in 1..256, got {M}")
        if B < 1 or T_out < 1:
            raise L.BsedError(f"Scaler.{who}: empty batch ({B} clips of {T_out} frames)")
        L._require_gpu()
        if self._acc is None:
            self._acc = torch.zeros((2, M), device=device, dtype=torch.float64)
        elif self._acc.device != device:
            raise L.BsedError(f"Scaler.{who}: the accumulator lives on {self._acc.device}, the batch on {device}")
        self._frames += int(B) * int(T_out)
        self.mean_ = self.mean_of_square_ = self.std_ = None
        self._dev = {}

    def _check_update_shape(self, who, T_out, M):
        """the first update asked for fixes (frames per clip, n_mels); the reference raises on differing shapes too"""
        if self._shape is None:
            self._shape = (int(T_out), int(M))
        elif self._shape != (int(T_out), int(M)):
            raise L.BsedError(f"Scaler.{who}: every update must have the same frame count and n_mels; had "
                              f"{self._shape}, got {(int(T_out), int(M))}")

    def update(self, mel_lin, clip_max=None, max_frames=None, top_db=80.0):
        """add LINEAR mel (B, T, n_mels) on the GPU, seen as the dB feature ``MelFrontEnd.to_db(mel_lin, clip_max,
        max_frames)`` would give; ``clip_max`` (B,) as ``MelFrontEnd.stats`` computes it when absent"""
        if not isinstance(mel_lin, torch.Tensor) or mel_lin.dim() != 3:
            raise L.BsedError("Scaler.update takes linear mel shaped (B, T, n_mels) as a GPU tensor")
        B, T, M = mel_lin.shape
        T_out = T if max_frames is None else int(max_frames)
        self._check_update_shape("update", T_out, M)
        if not mel_lin.is_cuda:
            raise L.BsedError("Scaler.update takes a GPU tensor (Scaler.normalize is the part that runs on the CPU)")
        self._begin("update", B, T_out, M, mel_lin.device)
        mel_lin = mel_lin.contiguous()
        if clip_max is None:
            clip_max = torch.empty((B,), device=mel_lin.device, dtype=torch.float32)
            sumsq = torch.empty((B, M), device=mel_lin.device, dtype=torch.float32)
            L.call("bsed_mel_stats", L.ptr(mel_lin), B, T, M, L.ptr(clip_max), L.ptr(sumsq), L.stream())
        scratch = torch.empty((L.lib().bsed_scaler_scratch_doubles(B, T, T_out, M),), device=mel_lin.device,
                              dtype=torch.float64)
        # algorithmic work: the rows that count are read once (the logarithm as ~20 operations per element)
        ops._note("scaler_accum_kernel<0>", f"T{T_out}", 24.0 * B * min(T, T_out) * M, 4.0 * B * min(T, T_out) * M)
        L.call("bsed_scaler_accum", L.ptr(mel_lin), L.ptr(clip_max), B, T, T_out, M, float(top_db),
               L.ptr(self._acc, torch.float64), L.ptr(scratch, torch.float64), L.stream())
        return self

    def update_db(self, x):
        """add a dB tensor (B, 1, T_out, n_mels) or (B, T_out, n_mels) on the GPU (already transformed features)"""
        if not isinstance(x, torch.Tensor) or x.dim() not in (3, 4) or (x.dim() == 4 and x.shape[1] != 1):
            raise L.BsedError("Scaler.update_db takes a dB tensor shaped (B, 1, T_out, n_mels) or (B, T_out, n_mels)")
        B, T_out, M = x.shape[0], x.shape[-2], x.shape[-1]
        self._check_update_shape("update_db", T_out, M)
        if not x.is_cuda:
            raise L.BsedError("Scaler.update_db takes a GPU tensor (Scaler.normalize is the part that runs on the CPU)")
        self._begin("update_db", B, T_out, M, x.device)
        x = x.contiguous()
        scratch = torch.empty((L.lib().bsed_scaler_scratch_doubles(B, T_out, T_out, M),), device=x.device,
                              dtype=torch.float64)
        ops._note("scaler_accum_kernel<1>", f"T{T_out}", 4.0 * B * T_out * M, 4.0 * B * T_out * M)
        L.call("bsed_scaler_accum_db", L.ptr(x), B, T_out, M, L.ptr(self._acc, torch.float64),
               L.ptr(scratch, torch.float64), L.stream())
        return self

    def update_waves(self, wav, frontend, max_frames=None):
        """add waveforms (B, n) on the GPU: ``frontend.linear`` followed by ``update`` (``max_frames`` None: the
        clips' own frame count, as ``SEDTrainer`` transforms them)"""
        mel, cmax, _ = frontend.linear(wav)
        return self.update(mel, cmax, max_frames=max_frames, top_db=frontend.cfg.top_db)

    def merge(self, other):
        """add another unfinished accumulator (sums and counts): sharded passes over one data set"""
        if other._acc is None:
            return self
        if self._shape is not None and self._shape != other._shape:
            raise L.BsedError(f"Scaler.merge: shapes differ: {self._shape} against {other._shape}")
        if self._acc is None:
            self._acc, self._shape = other._acc.clone(), other._shape
        else:
            self._acc += other._acc.to(self._acc.device)
        self._frames += other._frames
        self.mean_ = self.mean_of_square_ = self.std_ = None
        self._dev = {}
        return self

    def finish(self):
        """read the accumulator (the one host sync) -> (mean_, std_)"""
        if self._acc is None or self._frames == 0:
            raise L.BsedError("Scaler.finish: nothing was accumulated")
        acc = self._acc.cpu().numpy()
        self._set(acc[0] / self._frames, acc[1] / self._frames, "finish")
        return self.mean_, self.std_

    def calculate_scaler(self, dataset, frontend=None, max_frames=None, batch=64):
        """The reference's ``calculate_scaler`` -> (mean_, std_).  Items are ``((features, target), path)`` or
        ``(features, target)``.  Without ``frontend`` the features are dB tensors as the reference's transformed data
        sets give them ((1, T, n_mels) or (T, n_mels)).  With ``frontend`` they are LINEAR mel (T, n_mels) as
        ``FeatureDataset(transform=None)`` gives them, grouped by length as ``GpuCollate`` groups them so that each
        clip keeps its own top_db clamp, and seen padded / truncated to ``max_frames`` (default: the front end's)."""
        L._require_gpu()
        if frontend is not None and max_frames is None:
            max_frames = frontend.cfg.max_frames
        pending = {}

        def flush(key):
            feats = pending.pop(key)
            x = torch.from_numpy(np.stack(feats)).cuda()
            if frontend is None:
                self.update_db(x)
            else:
                self.update(x, max_frames=max_frames, top_db=frontend.cfg.top_db)

        for item in dataset:
            first = item[0]
            feats = first[0] if isinstance(first, (tuple, list)) else first
            if isinstance(feats, torch.Tensor):
                feats = feats.detach().cpu().numpy()
            feats = np.asarray(feats, dtype=np.float32)
            if frontend is None:
                feats = feats.reshape((-1,) + feats.shape[-1:]) if feats.ndim != 3 else feats[0]
            elif feats.ndim != 2:
                raise L.BsedError(f"calculate_scaler(frontend=...): features must be linear mel (T, n_mels), got {feats.shape}")
            self._check_update_shape("calculate_scaler", feats.shape[0] if frontend is None else max_frames, feats.shape[1])
            key = feats.shape
            pending.setdefault(key, []).append(feats)
            if len(pending[key]) >= batch:
                flush(key)
        for key in list(pending):
            flush(key)
        return self.finish()

    # ---- the statistics themselves ----------------------------------------------------------------------------------
    def _set(self, mean, mean_of_square, who):
        mean = np.ascontiguousarray(mean, dtype=np.float64)
        mean_of_square = np.ascontiguousarray(mean_of_square, dtype=np.float64)
        if mean.ndim != 1 or mean.shape != mean_of_square.shape or mean.size == 0:
            raise L.BsedError(f"Scaler.{who}: mean_ and mean_of_square_ must be two vectors of one length")
        std, bad = _bad_bands(mean, mean_of_square)
        if bad.size:
            raise L.BsedError(f"Scaler.{who}: no usable standard deviation in band(s) {bad.tolist()} "
                              f"(std_ {std[bad][:8].tolist()}): zero, negative variance or not finite")
        self.mean_, self.mean_of_square_, self.std_ = mean, mean_of_square, std
        self._dev = {}

    def check(self, n_mels=None, who="check"):
        """raise BsedError unless the statistics are set, usable and (if given) ``n_mels`` wide"""
        if self.std_ is None:
            raise L.BsedError(f"Scaler.{who}: no statistics yet (finish(), calculate_scaler() or load first)")
        std, bad = _bad_bands(np.asarray(self.mean_, dtype=np.float64), np.asarray(self.mean_of_square_, dtype=np.float64))
        bad = np.union1d(bad, np.flatnonzero(~(np.isfinite(self.std_) & (np.asarray(self.std_) > 0))))
        if bad.size:
            raise L.BsedError(f"Scaler.{who}: no usable standard deviation in band(s) {bad.tolist()}: zero, negative "
                              "variance or not finite")
        if n_mels is not None and len(self.mean_) != n_mels:
            raise L.BsedError(f"Scaler.{who}: statistics of {len(self.mean_)} bands for features of {n_mels}")

    def device_vectors(self, device="cuda"):
        """(mean_, std_) as float64 vectors on ``device``, uploaded once per device"""
        device = torch.device(device)
        if device.type == "cuda" and device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        v = self._dev.get(device)
        if v is None:
            self.check(who="device_vectors")
            v = self._dev[device] = (torch.from_numpy(self.mean_).to(device), torch.from_numpy(self.std_).to(device))
        return v

    def normalize(self, batch):
        """(batch - mean_) / std_ over the last axis.  GPU tensor: one launch, float32.  CPU tensor: numpy float64
        arithmetic and ``torch.Tensor(...)``'s cast to float32, as the reference.  numpy array: the float64 array the
        reference returns."""
        self.check(who="normalize")
        if isinstance(batch, torch.Tensor) and batch.is_cuda:
            if batch.dtype != torch.float32 or batch.shape[-1] != len(self.mean_):
                raise L.BsedError(f"Scaler.normalize: expected float32 (..., {len(self.mean_)}), got {batch.dtype} "
                                  f"{tuple(batch.shape)}")
            x = batch.contiguous()
            out = torch.empty_like(x)
            if x.numel() == 0:
                return out
            mean, std = self.device_vectors(x.device)
            M = x.shape[-1]
            ops._note("scaler_normalize_kernel", f"M{M}", 3.0 * x.numel(), 8.0 * x.numel())
            L.call("bsed_scaler_normalize", L.ptr(x), x.numel() // M, M, L.ptr(mean, torch.float64),
                   L.ptr(std, torch.float64), L.ptr(out), L.stream())
            return out
        if isinstance(batch, torch.Tensor):
            return torch.from_numpy(((batch.numpy() - self.mean_) / self.std_).astype(np.float32))
        return (batch - self.mean_) / self.std_

    # ---- persistence (the reference's format) -----------------------------------------------------------------------
    def state_dict(self):
        if type(self.mean_) is not np.ndarray:
            raise L.BsedError("Scaler.state_dict: no statistics yet")
        return {"mean_": self.mean_.tolist(), "mean_of_square_": self.mean_of_square_.tolist()}

    def load_state_dict(self, state_dict):
        self._set(np.array(state_dict["mean_"], dtype=np.float64), np.array(state_dict["mean_of_square_"], dtype=np.float64),
                  "load_state_dict")
        return self

    def save(self, path):
        with open(path, "w") as f:
            json.dump(self.state_dict(), f)

    def load(self, path):
        with open(path, "r") as f:
            self.load_state_dict(json.load(f))
        return self
