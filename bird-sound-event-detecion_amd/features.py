"""Mel front end on the GPU -- host-side mirror of the reference's feature code.

  preprocess(audio, compute_log=False)   <- reference src/data/preprocess.py:18-45
  MelFrontEnd.transform(...)             <- get_transforms(): AugmentGaussianNoise -> ApplyLog ->
                                            PadOrTrunc -> ToTensor (src/data/Transforms.py:304-322)

The reference runs these per clip on the CPU (librosa, offline + DataLoader).  Here a whole batch of
raw waveforms goes through three HIP kernels (csrc/mel.hip) and comes out as the (B,1,T,128) CRNN
input without leaving HBM.

  load_audio(path, sr)                   <- librosa.load(path, sr=cfg.sr) (src/data/preprocess.py:182): the file's PCM16
  Resampler(sr_in, sr_out)(x)               frames are uploaded as they are and mixed to mono and resampled by ONE kernel
  resample_filter(sr_in, sr_out)            (csrc/resample.hip).  The filter is this project's own Kaiser-windowed sinc,
                                            fully specified in ``resample_filter``; it is NOT librosa's (soxr's)
                                            resampler and no bit parity with it is claimed.

  loudness(waves, sr)                    ITU-R BS.1770-4 integrated loudness (LUFS) of every row of a batch, and the rows
  normalize_loudness(waves, sr, target)     scaled to a target (csrc/loudness.hip; the rules are include/bsed.h's: what
                                            scaper levels the reference's SYN set by, its values not pinned).
"""
import ctypes
import math

import numpy as np
import torch

from . import _lib as L
from . import ops


class MelConfig:
    """Constants of reference src/data/config.py:47-57 (``R`` config) as defaults."""

    def __init__(self, sr=32000, n_window=2048, hop_size=255, n_mels=128, mel_f_min=0.0, mel_f_max=None,
                 max_len_seconds=10.0, noise_snr=30.0, top_db=80.0):
        self.sr, self.n_window, self.hop_size, self.n_mels = sr, n_window, hop_size, n_mels
        self.mel_f_min = mel_f_min
        self.mel_f_max = min(16000.0, sr / 2.0) if mel_f_max is None else mel_f_max
        self.max_len_seconds, self.noise_snr, self.top_db = max_len_seconds, noise_snr, top_db

    @property
    def max_frames(self):
        return math.ceil(self.max_len_seconds * self.sr / self.hop_size)


class MelFrontEnd:
    """``scaler``: a ``scaler.Scaler`` with statistics (the reference's ``Normalize(scaler)``, the last transform of
    ``get_transforms``).  With one attached, ``to_db``, ``to_db_views`` and ``transform`` return normalised features from
    the same single launch (the dB kernels' NORM epilogue); ``linear``, ``stats``, ``add_noise`` and the module-level
    ``preprocess`` are untouched by it."""

    def __init__(self, cfg=None, scaler=None):
        L._require_gpu()
        self.cfg = cfg or MelConfig()
        self.scaler, self._norm = None, None
        c = L.STRUCTS["BsedMelCfg"](self.cfg.sr, self.cfg.n_window, self.cfg.hop_size, self.cfg.n_mels,
                                    self.cfg.mel_f_min, self.cfg.mel_f_max)
        self._plan = ctypes.c_void_p()
        L.call("bsed_mel_plan_create", ctypes.byref(c), ctypes.byref(self._plan))
        self.nnz = int(L.lib().bsed_mel_plan_nnz(self._plan))
        self.frames_per_wave = int(L.lib().bsed_mel_plan_frames_per_wave(self._plan))   # 2: stft_mel2_kernel
        self.set_scaler(scaler)

    def set_scaler(self, scaler):
        """attach a ``Scaler`` (or detach with None).  Its statistics are checked (BsedError names unusable bands) and the
        float64 device vectors are uploaded HERE, never inside ``to_db``: a captured training step contains no
        host-to-device copy.  Statistics changed later reach the front end through another ``set_scaler``."""
        if scaler is None:
            self.scaler, self._norm = None, None
            return
        scaler.check(self.cfg.n_mels, who="attach")
        mean, std = scaler.device_vectors(torch.device("cuda", torch.cuda.current_device()))
        self.scaler, self._norm = scaler, (L.ptr(mean, torch.float64), L.ptr(std, torch.float64), mean, std)

    def __del__(self):
        try:
            if getattr(self, "_plan", None):
                L.lib().bsed_mel_plan_destroy(self._plan)
                self._plan = None
        except Exception:
            pass

    def num_frames(self, n_samples):
        return 1 + n_samples // self.cfg.hop_size

    def linear(self, wav):
        """(B, n) float32 GPU waveforms -> (mel_lin (B,T,n_mels), clip_max (B,), bin_sumsq (B,n_mels))."""
        if wav.dim() == 1:
            wav = wav[None]
        B, n = wav.shape
        T = self.num_frames(n)
        mel = torch.empty((B, T, self.cfg.n_mels), device=wav.device, dtype=torch.float32)
        cmax = torch.empty((B,), device=wav.device, dtype=torch.float32)
        sumsq = torch.empty((B, self.cfg.n_mels), device=wav.device, dtype=torch.float32)
        # algorithmic work: wave in + linear mel out; per frame a 2048-point real FFT (2.5 N log2 N), 1025
        # magnitudes and the sparse filterbank
        ops._note("stft_mel2_kernel" if self.frames_per_wave == 2 else "stft_mel_kernel", f"T{T}",
                  B * T * (2.5 * 2048 * 11 + 4.0 * 1025 + 2.0 * self.nnz),
                  4.0 * B * (n + T * self.cfg.n_mels))
        scratch = torch.empty(L.lib().bsed_mel_scratch_floats(self._plan, B, n), device=wav.device, dtype=torch.float32)
        L.call("bsed_mel_linear", self._plan, L.ptr(wav), B, n, L.ptr(mel), L.ptr(cmax), L.ptr(sumsq), L.ptr(scratch),
               L.stream())
        return mel, cmax, sumsq

    def stats(self, mel_lin):
        """(clip_max (B,), bin_sumsq (B,n_mels)) of a linear-mel batch (for features loaded from .npy files)"""
        B, T, M = mel_lin.shape
        cmax = torch.empty((B,), device=mel_lin.device, dtype=torch.float32)
        sumsq = torch.empty((B, M), device=mel_lin.device, dtype=torch.float32)
        L.call("bsed_mel_stats", L.ptr(mel_lin), B, T, M, L.ptr(cmax), L.ptr(sumsq), L.stream())
        return cmax, sumsq

    def to_db(self, mel_lin, clip_max, max_frames=None):
        """linear mel -> dB with the per-clip top_db clamp, zero-padded / truncated to ``max_frames`` (0 dB pad rows);
        with a scaler attached every element is then ``float32((float64(v) - mean_) / std_)`` (a pad row: -mean_/std_)"""
        B, T, M = mel_lin.shape
        T_out = T if max_frames is None else max_frames
        out = torch.empty((B, 1, T_out, M), device=mel_lin.device, dtype=torch.float32)
        if self._norm is not None:
            # the same traffic plus the two float64 vectors; ~40 float64 operations per element for the division
            ops._note("mel_db_kernel<norm>", f"T{T_out}", 44.0 * B * T_out * M, 4.0 * B * M * (min(T, T_out) + T_out) + 16.0 * M)
            L.call("bsed_mel_db_norm", L.ptr(mel_lin), L.ptr(clip_max), B, T, T_out, M, self.cfg.top_db,
                   self._norm[0], self._norm[1], L.ptr(out), L.stream())
            return out
        ops._note("mel_db_kernel", f"T{T_out}", 4.0 * B * T_out * M, 4.0 * B * M * (T + T_out))
        L.call("bsed_mel_db", L.ptr(mel_lin), L.ptr(clip_max), B, T, T_out, M, self.cfg.top_db,
               L.ptr(out), L.stream())
        return out

    @staticmethod
    def _shifts(v, B, dev):
        """per-sample rolls as an int32 device tensor (B): a sequence of ints, or such a tensor passed through"""
        t = v if isinstance(v, torch.Tensor) else torch.as_tensor([int(s) for s in v], dtype=torch.int32)
        if t.dtype != torch.int32 or t.numel() != B:
            raise L.BsedError(f"per-sample shifts must be {B} int32 values, got {tuple(t.shape)} {t.dtype}")
        return t.to(dev).contiguous()

    def to_db_views(self, mel_lin, clip_max, shift_frames, shift_bins, max_frames=None):
        """``to_db`` plus the two rolled views of the ISP step from ONE read of the linear mel (``mel_db_views_kernel``):
        (x, x rolled per sample along time by shift_frames[b], x rolled along frequency by shift_bins[b]), the rolls
        being ``torch.roll`` of the padded / truncated (max_frames, n_mels) tensor as the reference applies them after
        ``PadOrTrunc`` (src/main_scmt_ada_weak.py:234-248).  Bitwise ``to_db`` followed by ``ops.roll``."""
        B, T, M = mel_lin.shape
        T_out = T if max_frames is None else max_frames
        sh, sw = self._shifts(shift_frames, B, mel_lin.device), self._shifts(shift_bins, B, mel_lin.device)
        outs = tuple(torch.empty((B, 1, T_out, M), device=mel_lin.device, dtype=torch.float32) for _ in range(3))
        if self._norm is not None:
            ops._note("mel_db_views_kernel<norm>", f"T{T_out}", 44.0 * B * T_out * M,
                      4.0 * B * M * (min(T, T_out) + 3 * T_out) + 16.0 * M)
            L.call("bsed_mel_db_views_norm", L.ptr(mel_lin), L.ptr(clip_max), B, T, T_out, M, self.cfg.top_db,
                   L.ptr(sh, torch.int32), L.ptr(sw, torch.int32), self._norm[0], self._norm[1], L.ptr(outs[0]),
                   L.ptr(outs[1]), L.ptr(outs[2]), L.stream())
            return outs
        ops._note("mel_db_views_kernel", f"T{T_out}", 4.0 * B * T_out * M, 4.0 * B * M * (T + 3 * T_out))
        L.call("bsed_mel_db_views", L.ptr(mel_lin), L.ptr(clip_max), B, T, T_out, M, self.cfg.top_db,
               L.ptr(sh, torch.int32), L.ptr(sw, torch.int32), L.ptr(outs[0]), L.ptr(outs[1]), L.ptr(outs[2]), L.stream())
        return outs

    def add_noise(self, mel_lin, bin_sumsq, seed=0, unit_noise=None):
        B, T, M = mel_lin.shape
        noisy = torch.empty_like(mel_lin)
        cmax = torch.empty((B,), device=mel_lin.device, dtype=torch.float32)
        ops._note("mel_noise_kernel", f"T{T}", 30.0 * B * T * M, 8.0 * B * T * M)
        L.call("bsed_mel_noise", L.ptr(mel_lin), L.ptr(bin_sumsq), L.ptr(unit_noise), B, T, M,
               self.cfg.noise_snr, seed, L.ptr(noisy), L.ptr(cmax), L.stream())
        return noisy, cmax

    def transform(self, wav, max_frames=None, noisy=False, seed=0, unit_noise=None, views=None):
        """waveforms -> dB-mel CRNN input (B,1,max_frames,n_mels) [, noisy twin for the EMA teacher].
        views=(shift_frames, shift_bins): every returned input becomes the triple (x, x time-rolled, x frequency-rolled)
        of ``to_db_views`` (the ISP step's inputs, without a separate roll pass)."""
        max_frames = self.cfg.max_frames if max_frames is None else max_frames
        mel, cmax, sumsq = self.linear(wav)
        if views is None:
            db = lambda m, c: self.to_db(m, c, max_frames)
        else:
            sh, sw = (self._shifts(v, mel.shape[0], mel.device) for v in views)
            db = lambda m, c: self.to_db_views(m, c, sh, sw, max_frames)
        clean = db(mel, cmax)
        if not noisy:
            return clean
        nz, nmax = self.add_noise(mel, sumsq, seed=seed, unit_noise=unit_noise)
        return clean, db(nz, nmax)


_default = {}


def preprocess(audio, compute_log=False, cfg=None):
    """Drop-in for the reference ``preprocess``: one waveform (numpy or tensor) -> (T, n_mels) float32
    numpy array of LINEAR mel amplitude (dB if compute_log).  Never normalised: the reference's ``preprocess`` runs
    before any ``Scaler`` exists, and its cached front ends carry none."""
    import numpy as np
    cfg = cfg or MelConfig()
    key = (cfg.sr, cfg.n_window, cfg.hop_size, cfg.n_mels, cfg.mel_f_min, cfg.mel_f_max)
    fe = _default.get(key)
    if fe is None:
        fe = _default[key] = MelFrontEnd(cfg)
    wav = torch.as_tensor(np.asarray(audio, dtype=np.float32)).cuda()[None]
    mel, cmax, _ = fe.linear(wav)
    if compute_log:
        mel = fe.to_db(mel, cmax)[:, 0]
    return mel[0].cpu().numpy()


# ---------------------------------------------------------------------------------------------------------------------
# Resampling
# ---------------------------------------------------------------------------------------------------------------------
def resample_filter(sr_in, sr_out, rolloff=0.91, attenuation_db=100.0):
    """The low-pass of the polyphase resampler sr_in -> sr_out, designed on the host in float64 ->
    ``(taps, up, down, half_len)``: ``taps`` float64, odd length ``2 * half_len + 1``, symmetric.

      g = gcd(sr_in, sr_out), up = sr_out / g, down = sr_in / g, fs_up = sr_in * up, low = min(sr_in, sr_out)
      pass band to fp = rolloff * low / 2, stop band from fst = low / 2, cutoff fc = (fp + fst) / 2
      Kaiser window: beta = 0.1102 (A - 8.7), N = ceil((A - 8) / (2.285 * 2 pi (fst - fp) / fs_up)), half_len = (N + 1) // 2
      taps[k + half_len] = up * (2 fc / fs_up) * sinc(2 fc k / fs_up) * kaiser[k + half_len],   k = -half_len .. half_len

    The resampler is ``y[m] = sum_j x[j] * taps[m * down - j * up + half_len]`` over the j with the tap index in range and
    0 <= j < n_in (zero outside the signal), ``n_out = ceil(n_in * up / down)``; zero-phase: y[m] sits at input time
    m * down / up.  At the defaults the stop band is at -100 dB and the pass-band ripple below 2e-4 dB."""
    for name, v in (("sr_in", sr_in), ("sr_out", sr_out)):
        if isinstance(v, bool) or int(v) != v or int(v) < 1:
            raise L.BsedError(f"resample_filter: {name} must be a positive integer rate in Hz, got {v!r}")
    sr_in, sr_out, rolloff, A = int(sr_in), int(sr_out), float(rolloff), float(attenuation_db)
    if not 0.0 < rolloff < 1.0:
        raise L.BsedError(f"resample_filter: rolloff must lie inside (0, 1), got {rolloff}")
    if not 21.0 < A <= 160.0:
        raise L.BsedError(f"resample_filter: attenuation_db must lie in (21, 160] (Kaiser's formulas; float64), got {A}")
    g = math.gcd(sr_in, sr_out)
    up, down = sr_out // g, sr_in // g
    fs_up, low = float(sr_in) * up, float(min(sr_in, sr_out))
    fp, fst = rolloff * low / 2.0, low / 2.0
    fc = (fp + fst) / 2.0
    beta = 0.1102 * (A - 8.7)
    N = math.ceil((A - 8.0) / (2.285 * 2.0 * math.pi * (fst - fp) / fs_up))
    half_len = (N + 1) // 2
    k = np.arange(-half_len, half_len + 1, dtype=np.float64)
    taps = up * (2.0 * fc / fs_up) * np.sinc(2.0 * fc * k / fs_up) * np.kaiser(2 * half_len + 1, beta)
    return taps, up, down, half_len


def resample_table(taps, up, down, half_len):
    """``taps`` -> the (up, P) float32 table ``bsed_resample_poly`` reads, one row per output residue c = m % up:
    ``table[c, i] = taps[(c * down + half_len) % up + i * up]``, 0 past the filter's end; P = (2 * half_len) // up + 1."""
    taps = np.asarray(taps, dtype=np.float64)
    P = (2 * half_len) // up + 1
    idx = ((np.arange(up, dtype=np.int64) * down + half_len) % up)[:, None] + np.arange(P, dtype=np.int64)[None, :] * up
    table = np.where(idx < len(taps), taps[np.minimum(idx, len(taps) - 1)], 0.0)
    return np.ascontiguousarray(table, dtype=np.float32)


class Resampler:
    """sr_in -> sr_out for whole recordings on the GPU, with the mono mix and the int16 conversion inside the same
    kernel.  The filter (``resample_filter``) is designed once, on the host; the device table is made on first use.
    ``sr_in == sr_out`` is the convert / mix-only case (one tap of 1.0).

    ``rs(x)``: x a numpy array or a GPU tensor, int16 or float32, shaped (n,) or (n, channels) as a WAV file interleaves
    them -> (n_out,) float32 GPU tensor.  Mono float32 input with ``sr_in == sr_out`` is returned as it is."""

    def __init__(self, sr_in, sr_out, rolloff=0.91, attenuation_db=100.0):
        taps, self.up, self.down, self.half_len = resample_filter(sr_in, sr_out, rolloff, attenuation_db)
        self.sr_in, self.sr_out = int(sr_in), int(sr_out)
        if self.sr_in == self.sr_out:
            taps, self.half_len = np.ones(1), 0
        self.taps = taps
        self.table = resample_table(taps, self.up, self.down, self.half_len)      # host copy (up, P) float32
        self.taps_per_phase = self.table.shape[1]
        self._dev = {}

    def n_out(self, n_in):
        return -(-int(n_in) * self.up // self.down)

    @staticmethod
    def form(x):
        """host-side check of an input -> (n frames, channels); raises BsedError, touches no GPU"""
        if not isinstance(x, (np.ndarray, torch.Tensor)):
            raise L.BsedError(f"Resampler takes a numpy array or a GPU tensor, got {type(x).__name__}")
        dt = str(x.dtype).replace("torch.", "")
        if dt not in ("int16", "float32"):
            raise L.BsedError(f"Resampler takes int16 or float32 samples, got {dt}")
        if x.ndim not in (1, 2):
            raise L.BsedError(f"Resampler takes samples shaped (n,) or (n, channels), got shape {tuple(x.shape)}")
        n, channels = int(x.shape[0]), int(x.shape[1]) if x.ndim == 2 else 1
        if n < 1 or not 1 <= channels <= 64:
            raise L.BsedError(f"Resampler needs at least one frame of 1..64 channels, got shape {tuple(x.shape)}")
        return n, channels

    def passes_through(self, x):
        """mono (n,) float32 at the target rate: nothing to compute"""
        return self.sr_in == self.sr_out and x.ndim == 1 and str(x.dtype).replace("torch.", "") == "float32"

    def __call__(self, x):
        n, channels = self.form(x)
        L._require_gpu()
        if isinstance(x, np.ndarray):
            x = torch.from_numpy(np.ascontiguousarray(x)).cuda()
        elif not x.is_cuda:
            raise L.BsedError("Resampler takes a numpy array or a GPU tensor, got a CPU tensor")
        x = x.contiguous()
        if self.passes_through(x):
            return x
        table = self._dev.get(x.device)
        if table is None:
            table = self._dev[x.device] = torch.from_numpy(self.table).to(x.device)
        s16 = x.dtype == torch.int16
        n_out = self.n_out(n)
        out = torch.empty((n_out,), device=x.device, dtype=torch.float32)
        ops._note(f"resample_poly_kernel<{int(s16)}>", f"{self.up}/{self.down} ch{channels}", 2.0 * n_out * self.taps_per_phase,
                  float(n * channels * (2 if s16 else 4) + 4 * n_out + 4 * self.table.size))
        L.call("bsed_resample_poly", L.ptr(x, x.dtype), L.CONSTANTS["BSED_PCM_S16" if s16 else "BSED_PCM_F32"], n, channels,
               L.ptr(table), self.up, self.down, self.half_len, L.ptr(out), n_out, L.stream())
        return out


_resamplers = {}


def resampler(sr_in, sr_out, rolloff=0.91, attenuation_db=100.0):
    """the cached ``Resampler`` of a rate pair and quality (the filter design and the device table are made once)"""
    key = (int(sr_in), int(sr_out), float(rolloff), float(attenuation_db))
    rs = _resamplers.get(key)
    if rs is None:
        rs = _resamplers[key] = Resampler(*key)
    return rs


def load_audio(path, sr=32000, **quality):
    """Counterpart of the reference's ``librosa.load(path, sr=cfg.sr)``: a PCM16 WAV file -> (mono float32 GPU waveform at
    ``sr``, sr).  ``data.read_wav`` reads the frames, they are uploaded as int16 and one launch mixes, converts and
    resamples them.  ``quality``: ``rolloff`` / ``attenuation_db`` of ``resample_filter``.  The samples are those of this
    project's filter, not librosa's."""
    from .data import read_wav
    x, sr_in = read_wav(path)
    return resampler(sr_in, sr, **quality)(x), int(sr)


def _rows_f32(waves, sr, who):
    """(n,) or (B, n), numpy or GPU tensor, float32 or int16 -> a contiguous (B, n) float32 device tensor (int16 scaled by
    1 / 32768 on the device, as ``load_audio`` converts it)"""
    if not isinstance(waves, (np.ndarray, torch.Tensor)):
        raise L.BsedError(f"{who} takes a numpy array or a GPU tensor, got {type(waves).__name__}")
    dt = str(waves.dtype).replace("torch.", "")
    if dt not in ("int16", "float32"):
        raise L.BsedError(f"{who} takes int16 or float32 samples, got {dt}")
    if waves.ndim not in (1, 2) or min(waves.shape) < 1:
        raise L.BsedError(f"{who} takes waveforms shaped (n,) or (B, n) with at least one sample, got shape {tuple(waves.shape)}")
    L._require_gpu()
    if isinstance(waves, np.ndarray):
        waves = torch.from_numpy(np.ascontiguousarray(waves)).cuda()
    elif not waves.is_cuda:
        raise L.BsedError(f"{who} takes a numpy array or a GPU tensor, got a CPU tensor")
    rows = waves.contiguous().reshape(-1, waves.shape[-1])
    if rows.dtype == torch.int16:
        rows = resampler(sr, sr)(rows.reshape(-1)).reshape(rows.shape)          # the convert-only launch
    return rows


def loudness(waves, sr):
    """Integrated loudness of every waveform in LUFS: ITU-R BS.1770-4 for one channel (K-weighting, 400 ms blocks at a
    100 ms hop, the -70 LUFS and the relative -10 LU gates), by the rules include/bsed.h states for ``bsed_loudness``.
    waves: (n,) or (B, n), a numpy array or a GPU tensor, float32 or int16 -> (B,) float64 GPU tensor from one call of
    the entry point; a waveform with no block above -70 LUFS (silence) gives -inf; one shorter than half a second is
    measured over whole repetitions of itself.  Nothing waits for the device.  The values are this rule's: no parity with
    pyloudnorm's or scaper's numbers is pinned."""
    rows = _rows_f32(waves, sr, "loudness")
    B, n = rows.shape
    off = torch.arange(B, device=rows.device, dtype=torch.int64) * n
    length = torch.full((B,), n, device=rows.device, dtype=torch.int64)
    return ops.loudness(rows.reshape(-1), off, length, sr, n, samples=B * n)


def normalize_loudness(waves, sr, target_lufs):
    """Scale every waveform to ``target_lufs``: row * 10^((target - L) / 20) with L = ``loudness`` of the row, on the
    device; a row at -inf (silence) is left unchanged.  -> (scaled float32, of the input's shape; lufs (B,) float64: the
    loudness BEFORE scaling).  Nothing waits for the device."""
    rows = _rows_f32(waves, sr, "normalize_loudness")
    lufs = loudness(rows, sr)
    gain = torch.where(torch.isinf(lufs), torch.ones_like(lufs), torch.pow(10.0, (float(target_lufs) - lufs) / 20.0))
    scaled = rows * gain.to(torch.float32)[:, None]
    return scaled.reshape(tuple(waves.shape)), lufs
