"""Float64 restatement of the integrated loudness of include/bsed.h (bsed_loudness), sequentially: the K-weighting
coefficients from the rate, the signal of a segment (a short one tiled up to half a second), the two biquads through
``scipy.signal.lfilter`` from zero state, blocks of four hops by the integer hop boundaries l_j = (j * sr) // 10, and the
two gates.  The reference of tests/test_loudness_*.py and tests/test_synth_lufs_gpu.py; the rules are BS.1770-4's for one
channel, and nothing here compares against pyloudnorm or scaper."""
import math

import numpy as np

SHELF = dict(f0=1681.974450955533, G=3.999843853973347, Q=0.7071752369554196, vb_exp=0.4996667741545416)
HIGH_PASS = dict(f0=38.13547087602444, Q=0.5003270373238773)
ABS_GATE = -70.0
MARGIN = 1e-3           # LU: a case is decidable when every L_j lies further than this from both gates
BAR = 1e-6              # LU: what the kernel may differ by (include/bsed.h, "Accuracy")


def kweight_coefs(sr):
    """-> (b, a) of the shelf, (b, a) of the high-pass, each a float64 array of 3 (a[0] = 1)"""
    K = math.tan(math.pi * SHELF["f0"] / sr)
    Vh = 10.0 ** (SHELF["G"] / 20.0)
    Vb = Vh ** SHELF["vb_exp"]
    Q = SHELF["Q"]
    a0 = 1.0 + K / Q + K * K
    b1 = np.array([(Vh + Vb * K / Q + K * K) / a0, 2.0 * (K * K - Vh) / a0, (Vh - Vb * K / Q + K * K) / a0])
    a1 = np.array([1.0, 2.0 * (K * K - 1.0) / a0, (1.0 - K / Q + K * K) / a0])
    K = math.tan(math.pi * HIGH_PASS["f0"] / sr)
    Q = HIGH_PASS["Q"]
    a0 = 1.0 + K / Q + K * K
    b2 = np.array([1.0, -2.0, 1.0])
    a2 = np.array([1.0, 2.0 * (K * K - 1.0) / a0, (1.0 - K / Q + K * K) / a0])
    return (b1, a1), (b2, a2)


def coefs10(sr):
    """the ten numbers ``bsed_kweight_coefs`` writes: b0 b1 b2 a1 a2 of stage 1, then of stage 2"""
    (b1, a1), (b2, a2) = kweight_coefs(sr)
    return np.concatenate([b1, a1[1:], b2, a2[1:]])


def n_eff(length, sr):
    half = (sr + 1) // 2
    return length if length >= half else length * -(-half // length)


def signal(x, off, length, sr, max_len=None):
    """v of the segment (off, length) of the flat buffer x, in float64: tiled to n_eff, zero outside the buffer"""
    x = np.asarray(x)
    if max_len is not None:
        length = min(length, max_len)
    idx = off + np.arange(n_eff(length, sr), dtype=np.int64) % length
    inside = (idx >= 0) & (idx < len(x))
    v = np.zeros(len(idx))
    v[inside] = x[idx[inside]].astype(np.float64)
    return v


def block_energies(v, sr):
    """z_j of the K-weighted v: the mean of y^2 over [l_j, l_(j+4)), for every block with l_(j+4) <= len(v)"""
    from scipy.signal import lfilter
    (b1, a1), (b2, a2) = kweight_coefs(sr)
    y = lfilter(b2, a2, lfilter(b1, a1, np.asarray(v, dtype=np.float64)))
    e = y * y
    z, j = [], 0
    while ((j + 4) * sr) // 10 <= len(v):
        lo, hi = (j * sr) // 10, ((j + 4) * sr) // 10
        z.append(e[lo:hi].sum() / (hi - lo))
        j += 1
    return np.array(z)


def gated(z):
    """-> (loud, [blocks, |A|, |G|], margin): margin = the smallest distance of any L_j to a gate it is compared with"""
    z = np.asarray(z, dtype=np.float64)
    with np.errstate(divide="ignore"):
        L = -0.691 + 10.0 * np.log10(z)
    finite = np.isfinite(L)
    margin = float(np.abs(L[finite] - ABS_GATE).min()) if finite.any() else math.inf
    A = L > ABS_GATE
    if not A.any():
        return -math.inf, [len(z), 0, 0], margin
    gamma = -0.691 + 10.0 * math.log10(z[A].mean()) - 10.0
    margin = min(margin, float(np.abs(L[A] - gamma).min()))
    G = A & (L > gamma)
    return -0.691 + 10.0 * math.log10(z[G].mean()), [len(z), int(A.sum()), int(G.sum())], margin


def loudness_ref(x, off, length, sr, max_len=None):
    """one segment -> (loud, counts, margin).  length < 1: (-inf, [0, 0, 0], inf)"""
    if length < 1:
        return -math.inf, [0, 0, 0], math.inf
    return gated(block_energies(signal(x, off, length, sr, max_len), sr))


def loudness_of(wave, sr):
    """a whole 1-D float array as one segment"""
    wave = np.asarray(wave)
    return loudness_ref(wave, 0, len(wave), sr)


def assert_decidable(margin, what=""):
    """the case does not sit on a gate: its counts and its value are then fixed by the rules to within round-off"""
    assert margin > MARGIN, f"{what}: a block lies {margin:.2e} LU from a gate (needs more than {MARGIN})"


def three_level_noise(sr, seed=0, seconds=(3.0, 4.0, 3.0), levels=(0.2, 0.002, 1e-5)):
    """Gaussian noise at three levels: above both gates, below the relative gate, below the absolute gate"""
    rng = np.random.default_rng(seed)
    return np.concatenate([(a * rng.standard_normal(int(round(s * sr)))) for s, a in zip(seconds, levels)]).astype(np.float32)


# ---- the cases of tests/test_loudness_gpu.py: one flat buffer per rate, segments at odd offsets that overlap -------------
LONGEST = 1000003                  # prime; 90 s at 11025 Hz, 23 s at 44100 Hz
PRIME = 100003
SIGNALS = ("noise", "silence", "sine", "noise_on_dc")          # the buffer ends in the loudest signal
SLACK = 4096                       # samples of a signal beyond the longest segment: room for the offsets


def gpu_buffer(sr):
    """Four signals of LONGEST + SLACK samples back to back -> (float32 buffer, {signal: its first sample}).  The
    three-level noise repeats every 10 s; "noise_on_dc" is the same noise on 0.5 + 0.3 sin(2 pi 20 t), whose DC and
    20 Hz content keep the high-pass ringing for thousands of samples: a split that carries too little state shows."""
    n = LONGEST + SLACK
    noise = np.resize(three_level_noise(sr, seed=sr), n)
    t = np.arange(n) / sr
    parts = {"noise": noise, "noise_on_dc": (noise + 0.5 + 0.3 * np.sin(2.0 * np.pi * 20.0 * t)).astype(np.float32),
             "sine": (0.25 * np.sin(2.0 * np.pi * 1234.5 * t)).astype(np.float32), "silence": np.zeros(n, np.float32)}
    base = {name: k * n for k, name in enumerate(SIGNALS)}
    return np.concatenate([parts[name] for name in SIGNALS]), base


def gpu_lengths(sr):
    half = (sr + 1) // 2
    return [1, 7, half - 1, half, half + sr // 10 - 1, half + sr // 10, 10 * sr, 10 * sr + 1, PRIME, LONGEST]


def gpu_segments(sr, base):
    """[(signal, offset, length), ...]: per signal eight offsets of each of the six short lengths, two of the next three
    and one of the longest -- 55 per signal, 220 in all; every offset is odd and segments of a signal overlap"""
    segs = []
    for name in SIGNALS:
        for k, length in enumerate(gpu_lengths(sr)):
            copies = 8 if k < 6 else 2 if k < 9 else 1
            segs += [(name, (base[name] + 2 * k + 502 * c) | 1, length) for c in range(copies)]
    return segs
