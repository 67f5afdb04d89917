"""tests/mel_reference.py, pinned without a GPU.

1. It equals oracle.mel_oracle at both product configurations, within what the oracle's own float32 steps cost:
     linear  the oracle stores the float64 spectrum as complex64 (modulus off by u = 2^-24), takes |.| in float32 (1 ulp =
             2 u) and multiplies by the basis in float32 (a dot product of nnz[m] non-negative terms in any order: nnz[m] u):
             (3 + nnz[m]) u ref.
     noise   the oracle's deviation is float32: x^2 (1), the scale (1), a mean of T terms in any order (T), the root
             (halves them, + 1): rel <= ((T + 2) / 2 + 1) u, + u for the float32 value of 10^(-snr/10) this reference takes.
     dB      clean view: float32 x^2 (10 log10(1 + u) = 4.35 u dB), numpy's float32 log10 (<= 4 ulp of the logarithm)
             times 10, and the float32 product: 4.35 u + 40 ulp32(ref / 10) + ulp32(ref).  Noisy view (float64 in the
             oracle, stored as float32): the noise bound carried through the logarithm on both sides of the value.
2. An honest float32 front end (torch.stft on the CPU, float32 basis product) stays inside mel_reference.linear_bound on
   every input family of tests/test_mel_kernels_gpu.py; the worst error / bound per family is printed.
3. Seven wrong front ends each leave the bound on at least one family: the bound discriminates.
4. Philox: the published Random123 known answers of Philox-4x32-10 (tests/golden/ holds no dropout words to compare
   with), the array form equals the integer form, and unit_normal's first two moments over 2^20 draws."""
import math

import numpy as np
import pytest
import torch

import mel_reference as R
from oracle import mel_oracle as mo

U = R.U
PRODUCT = [R.cfg(32000), R.cfg(22050)]
LENGTHS = [255 * 16 + 1, 255 * 32 + 17]


def _ulp32(x):
    return np.spacing(np.abs(np.asarray(x, np.float64)).astype(np.float32)).astype(np.float64)


# ------------------------------------------------------------------------------------------------ 1. the oracle
@pytest.mark.parametrize("c", PRODUCT, ids=lambda c: f"sr{c.sr}")
def test_reference_equals_oracle(c):
    y = mo.synth_clip(1, sr=c.sr, seconds=1.0)[0]
    W = R.basis(c)
    nnz = (W > 0).sum(-1)
    ref, S1, Wsum = R.linear(y, c, W)
    orc = mo.preprocess(y, sr=c.sr, fmax=c.fmax).astype(np.float64)
    T = 1 + len(y) // c.hop
    assert ref.shape == orc.shape == (T, 128)
    tol = (3.0 + nnz)[None, :] * U * ref
    assert (np.abs(orc - ref) <= tol).all(), float((np.abs(orc - ref) / tol).max())

    # noise and dB from the oracle's own float32 linear mel, so that only these stages are compared
    lin = orc.astype(np.float32)
    mx, sumsq, _ = R.stats(lin)
    assert mx == float(lin.max())
    z = np.random.default_rng(7).standard_normal(lin.shape).astype(np.float32)
    Tout = T + 5
    o_clean, o_noisy = mo.transform_pair(lin, Tout, unit_noise=z)
    r_clean, _ = R.db(lin, mx, 80.0, Tout)
    db_tol = lambda r: 4.35 * U + 40.0 * _ulp32(r / 10.0) + _ulp32(r)
    assert (np.abs(o_clean[0] - r_clean) <= db_tol(r_clean)).all()
    assert (o_clean[0, T:] == 0).all() and (r_clean[T:] == 0).all()
    sd = R.noise_sd(sumsq, T, 30.0)
    nz = R.noise(lin, sumsq, T, 30.0, z)
    dv = ((T + 2) / 2.0 + 2.0) * U * np.abs(z * sd[None, :])
    o_nz = mo.gaussian_noise(lin, 30.0, unit_noise=z)
    assert (np.abs(o_nz - nz) <= dv + 4 * np.spacing(np.abs(nz))).all()
    nmax = float(np.abs(o_nz).max())
    r_noisy, floor = R.db(nz, nmax, 80.0, Tout)
    hi, lo = R.db_raw(np.abs(nz) + dv), R.db_raw(np.maximum(np.abs(nz) - dv, 0.0))
    tol = np.zeros_like(r_noisy)
    tol[:T] = np.maximum(np.abs(np.maximum(hi, floor) - r_noisy[:T]), np.abs(np.maximum(lo, floor) - r_noisy[:T]))
    assert (np.abs(o_noisy[0] - r_noisy) <= tol + 2.0 * _ulp32(r_noisy) + 1e-6).all()
    # truncation
    assert np.array_equal(R.db(lin, mx, 80.0, T - 3)[0], r_clean[:T - 3])


def test_rolls_are_numpy_roll():
    a = np.arange(24.0).reshape(2, 3, 4)
    assert np.array_equal(R.roll_time(a, 4), np.roll(a, 1, axis=1))
    assert np.array_equal(R.roll_freq(a, -1), np.roll(a, 3, axis=2))


# ------------------------------------------------------------------------------------------------ 2./3. the bound
def _htk_basis(c):
    n_bins = 1 + R.N_FFT // 2
    to_mel = lambda f: 2595.0 * np.log10(1.0 + np.asarray(f, np.float64) / 700.0)
    to_hz = lambda m: 700.0 * (10.0 ** (np.asarray(m, np.float64) / 2595.0) - 1.0)
    mel_f = to_hz(np.linspace(to_mel(c.fmin), to_mel(c.fmax), c.n_mels + 2))
    fdiff = np.diff(mel_f)
    ramps = np.subtract.outer(mel_f, np.linspace(0.0, c.sr / 2.0, n_bins))
    w = np.zeros((c.n_mels, n_bins), np.float32)
    for i in range(c.n_mels):
        w[i] = np.maximum(0, np.minimum(-ramps[i] / fdiff[i], ramps[i + 2] / fdiff[i + 1]))
    return w


def _fp32_front_end(x, c, W32, pad_mode="reflect", periodic=False, offset=0, drop_last=False):
    """float32 STFT magnitude (torch.stft, CPU) times a float32 basis -> (T, n_mels) float64"""
    T = 1 + len(x) // c.hop
    half = R.N_FFT // 2
    pad = np.pad(x.astype(np.float32), (half, half + offset), mode=pad_mode)[offset:]
    win = np.hamming(R.N_FFT + 1)[:-1] if periodic else np.hamming(R.N_FFT)
    spec = torch.stft(torch.from_numpy(pad), R.N_FFT, hop_length=c.hop, window=torch.from_numpy(win.astype(np.float32)),
                      center=False, return_complex=True)
    mag = spec.abs()[:, :T].T.contiguous()                                   # (T, 1025) float32
    mel = (mag @ torch.from_numpy(np.ascontiguousarray(W32.T))).numpy().astype(np.float64)
    if drop_last:
        mel[-1] = 0.0                                                        # the frame is missing: nothing was written
    return mel


@pytest.fixture(scope="module")
def cases():
    """(cfg, n, family) -> (x, ref, bound), computed once"""
    out = {}
    for c in PRODUCT:
        W = R.basis(c)
        nnz = (W > 0).sum(-1)
        for n in LENGTHS:
            for name, x in R.families(n, c).items():
                ref, S1, Wsum = R.linear(x, c, W)
                out[(c, n, name)] = (x, ref, R.linear_bound(S1, Wsum, ref, nnz))
    return out


def _worst(cases, fn):
    """family -> worst error / bound over configurations and lengths (inf where the bound is 0 and the error is not)"""
    worst = {}
    for (c, n, name), (x, ref, bound) in cases.items():
        err = np.abs(fn(x, c) - ref)
        with np.errstate(divide="ignore", invalid="ignore"):
            ratio = np.where(err > 0, err / bound, 0.0)
        worst[name] = max(worst.get(name, 0.0), float(ratio.max()))
    return worst


def test_honest_fp32_front_end_is_inside_the_bound(cases):
    W32 = {c: mo.mel_filterbank(c.sr, R.N_FFT, c.n_mels, c.fmin, c.fmax) for c in PRODUCT}
    worst = _worst(cases, lambda x, c: _fp32_front_end(x, c, W32[c]))
    for name in sorted(worst):
        print(f"honest fp32 worst error / bound  {name:14s} {worst[name]:.4f}")
    assert set(worst) == set(R.families(LENGTHS[0], PRODUCT[0]))
    assert all(v < 1.0 for v in worst.values()), worst
    assert worst["zeros"] == 0.0


WRONG = {
    "zero padding": dict(pad_mode="constant"),
    "edge-replicate padding": dict(pad_mode="edge"),
    "periodic Hamming window": dict(periodic=True),
    "basis shifted by one bin": dict(shift_basis=True),
    "HTK mel scale": dict(htk=True),
    "frame t at t * hop + 1": dict(offset=1),
    "last frame dropped": dict(drop_last=True),
}


@pytest.mark.parametrize("what", sorted(WRONG))
def test_wrong_front_end_leaves_the_bound(cases, what):
    kw = dict(WRONG[what])
    shift, htk = kw.pop("shift_basis", False), kw.pop("htk", False)

    def basis32(c):
        if htk:
            return _htk_basis(c)
        W = mo.mel_filterbank(c.sr, R.N_FFT, c.n_mels, c.fmin, c.fmax)
        return np.roll(W, 1, axis=1) if shift else W

    W32 = {c: basis32(c) for c in PRODUCT}
    worst = _worst(cases, lambda x, c: _fp32_front_end(x, c, W32[c], **kw))
    top = max(worst, key=worst.get)
    print(f"wrong front end: {what:26s} worst error / bound {worst[top]:.3g} on {top}; "
          f"families outside: {sorted(k for k, v in worst.items() if v > 1.0)}")
    assert worst[top] > 1.0, worst


# ------------------------------------------------------------------------------------------------ 4. Philox
def test_philox_known_answers_and_structure():
    # Random123's published known-answer vectors of philox4x32-10 (kat_vectors)
    kat = [((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
           ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
           ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0),
            (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1))]
    for ctr, key, want in kat:
        assert R.philox4x32_10(ctr, key) == want
    # the wrapper's word order: counter lo / hi, stream, the fixed word; key = seed lo / hi
    seed, counter = (7 << 32) | 5, (3 << 32) | 9
    assert R.philox4x32(counter, R.NOISE_STREAM, seed) == R.philox4x32_10((9, 3, R.NOISE_STREAM, 0x5EED5EED), (5, 7))
    assert R.philox4x32(9, R.NOISE_STREAM, seed) != R.philox4x32(9, R.NOISE_STREAM, 5)
    # the array form is the integer form
    counters = np.array([0, 1, 2, 12345, (1 << 32) + 3, (1 << 40) - 1], np.uint64)
    words = R.philox4x32_array(counters, R.NOISE_STREAM, seed)
    for j, cn in enumerate(counters):
        assert tuple(int(w) for w in words[:, j]) == R.philox4x32(int(cn), R.NOISE_STREAM, seed)


def test_unit_normal_draws():
    n = 1 << 20
    gi = np.arange(n, dtype=np.uint64)
    z, rad, u1, u2 = R.unit_normal(gi, 1234, parts=True)
    assert np.isfinite(z).all() and (u1 > 0).all() and (u1 <= 1.0).all() and (u2 > 0).all()
    # both members of a counter pair share the uniforms; the even one takes the cosine, the odd one the sine
    assert np.array_equal(u1[0::2], u1[1::2]) and np.array_equal(u2[0::2], u2[1::2])
    np.testing.assert_allclose(z[0::2] ** 2 + z[1::2] ** 2, rad[0::2] ** 2, rtol=1e-12, atol=1e-300)
    assert z[0] == rad[0] * math.cos(2.0 * math.pi * u2[0]) and z[1] == rad[1] * math.sin(2.0 * math.pi * u2[1])
    # sampling error at 5 sigma: mean sd 1 / sqrt(n), variance sd sqrt(2 / n), cosine-sine correlation sd 1 / sqrt(n / 2)
    assert abs(z.mean()) < 5.0 / math.sqrt(n)
    assert abs(z.var() - 1.0) < 5.0 * math.sqrt(2.0 / n)
    assert abs((z[0::2] * z[1::2]).mean()) < 5.0 / math.sqrt(n / 2)
    assert not np.array_equal(z, R.unit_normal(gi, (7 << 32) | 1234))
    # u1 can round to exactly 1.0 (r >> 8 = 2^24 - 1): the draw is then 0, not a NaN or an infinity
    top = (np.float32(2 ** 24 - 1) + np.float32(0.5)) * np.float32(2.0 ** -24)
    assert top == np.float32(1.0) and math.sqrt(-2.0 * math.log(float(top))) == 0.0
