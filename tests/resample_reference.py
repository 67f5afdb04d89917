"""Float64 restatement of the polyphase resampler, the reference of tests/test_resample_cpu.py and
tests/test_resample_gpu.py:

    y[m] = sum_j x[j] * taps[m * down - j * up + half_len]     over 0 <= j < n_in and 0 <= tap index <= 2 * half_len

evaluated straight from that definition for any chosen set of output indices, together with S[m] = sum |x[j]| |tap| and
the number of terms K[m].  Fed with the fp32-rounded taps and the fp32 mono mix the kernel sees (``taps32``,
``mono_f32``), both promoted to float64, it differs from the kernel by the kernel's fp32 accumulation alone, which is
what the bound (K + 2) * 2^-24 * S measures."""
import numpy as np

RATE_PAIRS = [(48000, 32000), (44100, 32000), (44100, 22050), (48000, 22050), (16000, 32000), (22050, 32000)]
UP_DOWN = {(48000, 32000): (2, 3), (44100, 32000): (320, 441), (44100, 22050): (1, 2), (48000, 22050): (147, 320),
           (16000, 32000): (2, 1), (22050, 32000): (640, 441)}            # worked by hand
U24, U53 = 2.0 ** -24, 2.0 ** -53


def n_out(n_in, up, down):
    return -(-n_in * up // down)


def taps32(taps):
    """the taps as the device table holds them"""
    return np.asarray(taps, np.float64).astype(np.float32).astype(np.float64)


def mono_f32(x):
    """the mono sample of every frame exactly as include/bsed.h states it, in float32 arithmetic:
    int16: (float)(integer channel sum) * fp32(1 / (32768 * channels)); float32: the channels added in order, times
    fp32(1 / channels)"""
    x = np.asarray(x)
    x2 = x.reshape(len(x), -1)
    ch = x2.shape[1]
    if x.dtype == np.int16:
        return x2.astype(np.int32).sum(axis=1).astype(np.float32) * np.float32(1.0 / (32768.0 * ch))
    assert x.dtype == np.float32, x.dtype
    s = x2[:, 0].copy()
    for c in range(1, ch):
        s = (s + x2[:, c]).astype(np.float32)
    return (s * np.float32(1.0 / ch)).astype(np.float32)


def resample_ref(x, taps, up, down, half_len, idx=None, chunk=8192):
    """x (n_in,) mono, taps (2 * half_len + 1,) -> (y, S, K) in float64 / float64 / int64 at the output indices ``idx``
    (default: all n_out of them)"""
    x = np.asarray(x, dtype=np.float64)
    taps = np.asarray(taps, dtype=np.float64)
    n_in = len(x)
    assert len(taps) == 2 * half_len + 1
    m_all = np.arange(n_out(n_in, up, down), dtype=np.int64) if idx is None else np.asarray(idx, dtype=np.int64)
    P = (2 * half_len) // up + 1
    i = np.arange(P, dtype=np.int64)[None, :]
    y, S, K = (np.zeros(len(m_all)), np.zeros(len(m_all)), np.zeros(len(m_all), np.int64))
    for lo in range(0, len(m_all), chunk):
        m = m_all[lo:lo + chunk, None]
        q = m * down + half_len
        j = q // up - i                                  # the samples whose tap index q - j * up is >= 0, descending
        t = q - j * up
        ok = (t <= 2 * half_len) & (j >= 0) & (j < n_in)
        xv = np.where(ok, x[np.clip(j, 0, n_in - 1)], 0.0)
        tv = np.where(ok, taps[np.clip(t, 0, 2 * half_len)], 0.0)
        y[lo:lo + chunk] = (xv * tv).sum(axis=1)
        S[lo:lo + chunk] = (np.abs(xv) * np.abs(tv)).sum(axis=1)
        K[lo:lo + chunk] = ok.sum(axis=1)
    return y, S, K


def response_db(taps, up, sr_in, sr_out, rolloff=0.91, pad=16):
    """(worst stop-band level, pass-band ripple) in dB of taps / up on a ``pad``-times zero-padded FFT at rate sr_in * up"""
    n = pad * len(taps)
    H = np.abs(np.fft.rfft(np.asarray(taps) / up, n))
    f = np.arange(len(H)) * (sr_in * up / n)
    low = min(sr_in, sr_out)
    stop = 20 * np.log10(H[f >= low / 2].max())
    pb = 20 * np.log10(H[f <= rolloff * low / 2])
    return stop, max(pb.max(), -pb.min())
