"""The float64 restatement of the integrated loudness (tests/loudness_reference.py) checked against what BS.1770-4 itself
fixes: the 48 kHz coefficient table, the level of a full-scale 997 Hz sine, the 20 LU of a tenfold amplitude, the two
gates on a three-level signal, silence, and the tiling and block count at the short lengths.  No GPU, no library call."""
import math

import numpy as np
import pytest

import loudness_reference as lr


def test_coefficients_at_48_khz_are_the_standards_table():
    (b1, a1), (b2, a2) = lr.kweight_coefs(48000)
    assert np.abs(b1 - [1.53512485958697, -2.69169618940638, 1.19839281085285]).max() <= 1e-12
    assert np.abs(a1 - [1.0, -1.69065929318241, 0.73248077421585]).max() <= 1e-12
    assert b2.tolist() == [1.0, -2.0, 1.0]
    assert np.abs(a2 - [1.0, -1.99004745483398, 0.99007225036621]).max() <= 1e-12
    assert lr.coefs10(48000).shape == (10,) and lr.coefs10(48000)[3] == a1[1] and lr.coefs10(48000)[9] == a2[2]


def _sine(amplitude, sr=48000, seconds=20.0, f=997.0):
    return amplitude * np.sin(2.0 * np.pi * f * np.arange(int(seconds * sr)) / sr)


def test_full_scale_997_hz_sine_measures_minus_3_01_lufs_and_a_tenth_of_it_20_lu_less():
    loud, counts, margin = lr.loudness_of(_sine(1.0), 48000)
    print(f"997 Hz full scale: {loud:.6f} LUFS, counts {counts}, margin {margin:.3f} LU")
    assert abs(loud - (-3.01)) <= 0.01
    assert counts == [197, 197, 197]
    quiet, counts10, _ = lr.loudness_of(_sine(0.1), 48000)
    assert counts10 == counts and abs((loud - quiet) - 20.0) <= 1e-9


def test_three_levels_of_noise_give_three_different_counts():
    loud, counts, margin = lr.loudness_of(lr.three_level_noise(32000), 32000)
    print(f"three-level noise: {loud:.6f} LUFS, counts {counts}, margin {margin:.3f} LU")
    assert counts == [97, 70, 30]
    lr.assert_decidable(margin, "three-level noise")
    assert margin > 5.0
    # what survives both gates is the loud part: 27 blocks inside it and the three that hang 100, 200 and 300 ms over its
    # end, so the mean is (27 + 0.75 + 0.5 + 0.25) / 30 of the loud part's own: 0.22 LU less
    rng = np.random.default_rng(0)
    alone, _, _ = lr.loudness_of((0.2 * rng.standard_normal(3 * 32000)).astype(np.float32), 32000)
    assert abs(loud - (alone + 10.0 * math.log10(28.5 / 30.0))) <= 0.05


def test_silence_and_empty_segments_give_minus_infinity():
    loud, counts, margin = lr.loudness_of(np.zeros(32000, np.float32), 32000)
    assert loud == -math.inf and counts == [7, 0, 0] and margin == math.inf
    assert lr.loudness_ref(np.ones(10, np.float32), 0, 0, 32000) == (-math.inf, [0, 0, 0], math.inf)
    loud, counts, _ = lr.loudness_of(np.full(32000, 1e-6, np.float32) * np.resize([1, -1], 32000), 32000)
    assert loud == -math.inf and counts[0] == 7 and counts[1] == 0            # far below the absolute gate


def test_short_lengths_are_tiled_to_half_a_second_and_the_block_count_steps():
    sr, half = 32000, 16000
    x = (0.1 * np.random.default_rng(2).standard_normal(40000)).astype(np.float32)
    want = {1: (16000, 2), 7: (16002, 2), half - 1: (2 * (half - 1), 6), half: (half, 2), half + sr // 10 - 1: (half + 3199, 2),
            half + sr // 10: (half + 3200, 3)}
    for length, (n, blocks) in want.items():
        v = lr.signal(x, 5, length, sr)
        assert lr.n_eff(length, sr) == n == len(v)
        assert np.array_equal(v, np.resize(x[5:5 + length].astype(np.float64), n))
        loud, counts, _ = lr.loudness_ref(x, 5, length, sr)
        assert counts[0] == blocks and (math.isfinite(loud) or length == 1), length
    # outside the buffer reads zero; max_len cuts first
    assert np.array_equal(lr.signal(x, 39990, 20000, sr)[:12], np.concatenate([x[39990:], [0.0, 0.0]]))
    assert np.array_equal(lr.signal(x, -3, 16000, sr)[:5], np.concatenate([[0.0] * 3, x[:2]]))
    assert np.array_equal(lr.signal(x, 0, 30000, sr, max_len=100), np.resize(x[:100].astype(np.float64), 16000))


def test_uneven_hops_at_11025_hz():
    sr = 11025
    bounds = [(j * sr) // 10 for j in range(6)]
    assert bounds == [0, 1102, 2205, 3307, 4410, 5512] and {b - a for a, b in zip(bounds, bounds[1:])} == {1102, 1103}
    rng = np.random.default_rng(3)
    x = (0.1 * rng.standard_normal(3 * sr)).astype(np.float32)
    z = lr.block_energies(x.astype(np.float64), sr)
    assert len(z) == 27                                       # l_(j+4) <= 33075 while j <= 26
    assert len(lr.block_energies(x[:5512].astype(np.float64), sr)) == 2 and len(lr.block_energies(x[:5511].astype(np.float64), sr)) == 1
    loud, counts, margin = lr.loudness_of(x, sr)
    assert counts == [27, 27, 27] and margin > 1.0
    assert abs(loud - (-0.691 + 10.0 * math.log10(z.mean()))) <= 1e-12


@pytest.mark.parametrize("sr", [8000, 11025, 16000, 22050, 32000, 44100, 48000, 96000])
def test_high_pass_and_shelf_are_stable_and_shaped_as_k_weighting(sr):
    from scipy.signal import freqz
    (b1, a1), (b2, a2) = lr.kweight_coefs(sr)
    for a in (a1, a2):
        assert np.abs(np.roots(a)).max() < 1.0
    f = np.array([20.0, 1000.0, min(10000.0, 0.45 * sr)])
    h = np.abs(freqz(b1, a1, worN=f, fs=sr)[1] * freqz(b2, a2, worN=f, fs=sr)[1])
    db = 20.0 * np.log10(h)
    assert db[0] < -9.0 and abs(db[1] - 0.7) < 0.3 and 2.0 < db[2] < 4.5     # rumble cut, about 0.7 dB at 1 kHz, the shelf
