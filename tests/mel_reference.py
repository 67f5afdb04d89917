"""float64 restatement of the mel front end's contracts (include/bsed.h, "Mel front end": bsed_mel_linear, bsed_mel_stats,
bsed_mel_noise, bsed_mel_db, bsed_mel_db_views).  Plain numpy, no kernel structure: frames are gathered from the
reflect-padded clip, the spectrum is numpy's float64 rfft, the Slaney basis is the float32 table of
oracle.mel_oracle.mel_filterbank widened to float64 (its values are the operation's inputs), sums of squares are exactly
rounded (math.fsum).  The Philox counter generator of csrc/bsed_common.h is restated on integers; the uniform of
mel_noise_kernel is evaluated in numpy float32, where every step is exact or correctly rounded, and Box-Muller in float64.
tests/test_mel_reference_cpu.py pins this module against oracle.mel_oracle and shows which mistakes its bounds catch."""
import math
from collections import namedtuple

import numpy as np

from oracle import mel_oracle as mo

N_FFT = 2048
U = 2.0 ** -24

Cfg = namedtuple("Cfg", "sr hop n_mels fmin fmax")


def cfg(sr=32000, hop=255, n_mels=128, fmin=0.0, fmax=None):
    return Cfg(sr, hop, n_mels, float(fmin), float(min(16000.0, sr / 2.0) if fmax is None else fmax))


def f32(x):
    """the float32 value a scalar argument of the C ABI arrives as, as a Python float"""
    return float(np.float32(x))


# ---------------------------------------------------------------------------------------------- linear mel
def frames(x, hop):
    """(n,) -> (T, 2048) float64: reflect-centre padding of n_fft // 2, frame t starts at t * hop; T = 1 + n // hop"""
    x = np.asarray(x, np.float64)
    pad = np.pad(x, N_FFT // 2, mode="reflect")
    T = 1 + len(x) // hop
    idx = hop * np.arange(T)[:, None] + np.arange(N_FFT)[None, :]
    return pad[idx]


def basis(c):
    """(n_mels, 1025) float64: the float32 Slaney table, widened"""
    return mo.mel_filterbank(c.sr, N_FFT, c.n_mels, c.fmin, c.fmax).astype(np.float64)


def linear(x, c, W=None):
    """(n,) waveform -> (mel (T, n_mels), S1 (T,), Wsum (n_mels,)), all float64.
    S1[t] = sum_n |x_n| w_n over the padded frame: the magnitude sum a bound on the FFT's rounding is stated in.
    Wsum[m] = sum_k W[m, k]."""
    W = basis(c) if W is None else W
    fr = frames(x, c.hop)
    win = np.hamming(N_FFT)
    mag = np.abs(np.fft.rfft(fr * win[None, :], axis=-1))
    return mag @ W.T, (np.abs(fr) * win[None, :]).sum(-1), W.sum(-1)


# ---------------------------------------------------------------------------------------------- statistics
def stats(mel):
    """(T, n_mels) -> (max, sumsq (n_mels,), the same sums: squares are their own magnitudes), sums exactly rounded.
    The max starts from 0 as the kernels' does: linear mel is never negative."""
    mel = np.asarray(mel, np.float64)
    sq = mel * mel                                   # exact in float64 for float32 inputs
    s = np.array([math.fsum(sq[:, j]) for j in range(sq.shape[1])], np.float64)
    return max(float(mel.max()), 0.0), s, s.copy()


# ---------------------------------------------------------------------------------------------- noise
def snr_scale(snr_db):
    """10^(-snr/10) at the float32 value the kernel receives (the host's powf; its one rounding is the caller's to count)"""
    return float(np.float32(10.0 ** (-f32(snr_db) / 10.0)))


def noise_sd(sumsq, T, snr_db):
    return np.sqrt(np.asarray(sumsq, np.float64) / float(T) * snr_scale(snr_db))


def noise(mel, sumsq, T, snr_db, z):
    """mel + z * sqrt(sumsq / T * 10^(-snr/10)), broadcast over the band axis"""
    return np.asarray(mel, np.float64) + np.asarray(z, np.float64) * noise_sd(sumsq, T, snr_db)


M32 = 0xFFFFFFFF


def philox4x32_10(ctr, key):
    """Philox-4x32 with 10 rounds on Python integers: ctr = (c0, c1, c2, c3), key = (k0, k1) -> four 32-bit words"""
    c0, c1, c2, c3 = ctr
    k0, k1 = key
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c0, 0xCD9E8D57 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & M32, (p0 >> 32) ^ c3 ^ k1, p0 & M32
        k0, k1 = (k0 + 0x9E3779B9) & M32, (k1 + 0xBB67AE85) & M32
    return c0, c1, c2, c3


def philox4x32(counter, stream, seed):
    """csrc/bsed_common.h: counter words (lo, hi, stream, 0x5eed5eed), key = (seed lo, seed hi)"""
    return philox4x32_10((counter & M32, (counter >> 32) & M32, stream & M32, 0x5EED5EED), (seed & M32, (seed >> 32) & M32))


def philox4x32_array(counter, stream, seed):
    """the same on a uint64 numpy array of counters -> (4, n) uint64 holding 32-bit words"""
    counter = np.asarray(counter, np.uint64)
    m = np.uint64(M32)
    s32 = np.uint64(32)
    c0, c1 = counter & m, counter >> s32
    c2 = np.full_like(counter, stream & M32)
    c3 = np.full_like(counter, 0x5EED5EED)
    k0, k1 = seed & M32, (seed >> 32) & M32
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c0, np.uint64(0xCD9E8D57) * c2          # < 2^64: no wrap
        c0, c1, c2, c3 = (p1 >> s32) ^ c1 ^ np.uint64(k0), p1 & m, (p0 >> s32) ^ c3 ^ np.uint64(k1), p0 & m
        k0, k1 = (k0 + 0x9E3779B9) & M32, (k1 + 0xBB67AE85) & M32
    return np.stack([c0, c1, c2, c3])


NOISE_STREAM = 0x4E4F4953


def unit_uniforms(gi, seed):
    """the two uniforms of element gi's counter pair: u = fl32(fl32(r >> 8) + 0.5f) * 2^-24 in numpy float32.  r >> 8 is
    below 2^24 and converts exactly; the sum rounds to nearest even above 2^23 (so u1 can be exactly 1.0); the power of
    two is exact."""
    gi = np.asarray(gi, np.uint64)
    r = philox4x32_array(gi >> np.uint64(1), NOISE_STREAM, seed)
    u = [((w >> np.uint64(8)).astype(np.float32) + np.float32(0.5)) * np.float32(2.0 ** -24) for w in r[:2]]
    assert u[0].dtype == np.float32
    return u[0].astype(np.float64), u[1].astype(np.float64)


def unit_normal(gi, seed, parts=False):
    """mel_noise_kernel's draw for the global element index gi: Box-Muller on counter gi >> 1, cosine for even gi, sine
    for odd.  parts=True also returns (radius, u1, u2) for the caller's error budget."""
    gi = np.asarray(gi, np.uint64)
    u1, u2 = unit_uniforms(gi, seed)
    rad = np.sqrt(-2.0 * np.log(u1))
    ang = 2.0 * math.pi * u2
    z = np.where((gi & np.uint64(1)) == 1, rad * np.sin(ang), rad * np.cos(ang))
    return (z, rad, u1, u2) if parts else z


# ---------------------------------------------------------------------------------------------- dB
def db_raw(x):
    """10 log10(max(1e-10, x^2)) in float64 (no clamp)"""
    x = np.asarray(x, np.float64)
    return 10.0 * np.log10(np.maximum(1e-10, x * x))


def db(x, clip_max, top_db, T_out):
    """(T, n_mels) linear mel of one clip -> (T_out, n_mels): dB clamped at db_raw(clip_max) - top_db, rows past T are 0,
    rows past T_out dropped.  Also returns the floor."""
    x = np.asarray(x, np.float64)
    floor = float(db_raw(float(clip_max))) - f32(top_db)
    T = x.shape[0]
    out = np.zeros((T_out, x.shape[1]), np.float64)
    n = min(T, T_out)
    out[:n] = np.maximum(db_raw(x[:n]), floor)
    return out, floor


def roll_time(a, s):
    return np.roll(a, s, axis=-2)


def roll_freq(a, s):
    return np.roll(a, s, axis=-1)


# ---------------------------------------------------------------------------------------------- bound and test inputs
# Roundings along one path from a sample to a magnitude in csrc/mel.hip, each at most u = 2^-24 of the path's magnitude,
# counted on complex moduli (a complex add errs by u of its result, a complex product by at most 2 sqrt(2) u, held at 3; a
# table entry is off by at most u).  The larger count of the two kernels is taken at every stage:
#    2  window: the float32 table, the product
#   16  two 16-point DFTs, each: radix-4 level (2 adds), inner W16 twiddle (constant 1 + product 3), radix-4 level (2 adds)
#    8  twiddle W1024^(l k1): stft_mel2_kernel forms it as a product of two table entries (2 + 3), then the product (3);
#       stft_mel_kernel reads one entry (1 + 3)
#    4  twiddle W64^(m k2): table 1, product 3
#    2  radix-4 across the quad: two fused multiply-adds
#   10  real-FFT unpack: Z[k] +- conj Z[1024 - k] (1), W2048^k = table entry x folded constant (2 + 3), its product with
#       the odd part (3), E +- that (1)
#    3  magnitude: the sum of squares (2 roundings, halved by the root) 1, v_sqrt_f32 at 1 ulp = 2 u; the 0.5 is exact
D_FFT = 2 + 16 + 8 + 4 + 2 + 10 + 3


def linear_bound(S1, Wsum, ref, nnz):
    """|err[t, m]| <= D u S1[t] Wsum[m] + F[m] u ref[t, m].  Every magnitude is off by at most D u S1 (D_FFT above), and
    the filterbank adds F[m] = nnz[m] + 1: one fused multiply-add per non-zero weight of the band, each rounding a partial
    sum of non-negative terms (zero-weight padding steps are exact), plus the weight's own float32 rounding (the kernel's
    table is made by its own host code)."""
    return D_FFT * U * S1[:, None] * Wsum[None, :] + (np.asarray(nnz, np.float64)[None, :] + 1.0) * U * np.abs(ref)


def band_tone_hz(c, band):
    """a frequency half way between two FFT bins, next to the centre of a band"""
    centre = float(mo.mel_frequencies(c.n_mels + 2, c.fmin, c.fmax)[band + 1])
    binw = c.sr / float(N_FFT)
    return (math.floor(centre / binw) + 0.5) * binw


def families(n, c, seed=0):
    """name -> (n,) float32: the seeded input families of the mel tests"""
    rng = np.random.default_rng([seed, n])
    white = rng.uniform(-1.0, 1.0, n).astype(np.float32)
    i = np.arange(n, dtype=np.float64)
    out = {"white": white, "white_2^-20": white * np.float32(2.0 ** -20)}
    out["dc"] = np.full(n, 0.75, np.float32)
    out["nyquist"] = (0.75 * (1.0 - 2.0 * (i % 2))).astype(np.float32)                   # (-1)^n
    out["bin512"] = (0.75 * np.cos(0.5 * math.pi * (i % 4))).astype(np.float32)          # cos(pi n / 2), exact values
    for name, band in (("tone_top", c.n_mels - 1), ("tone_band0", 0)):
        out[name] = (0.75 * np.cos(2.0 * math.pi * band_tone_hz(c, band) / c.sr * i)).astype(np.float32)
    imp = np.zeros(n, np.float32)
    imp[(2 * n) // 3] = 1.0
    out["impulse"] = imp
    hdr = (1e-4 * rng.standard_normal(n))
    lo = n // 2
    hi = min(n, lo + 2000)
    hdr[lo:hi] += 0.9 * np.cos(2.0 * math.pi * 3000.0 / c.sr * i[lo:hi])
    out["hdr_burst"] = hdr.astype(np.float32)
    out["zeros"] = np.zeros(n, np.float32)
    return out
