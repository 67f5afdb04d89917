"""Soundscapes levelled by integrated loudness (``SoundBank(loudness="lufs")``, ``plan_soundscapes(loudness="lufs")``): the
bank's measurements against the sequential float64 restatement (tests/loudness_reference.py), a clip that is one whole
background against ``ref_db``, and a synthesized batch against the loudness of the float64 mix of the same plan
(tests/synth_reference.py)."""
import math

import numpy as np
import pytest
import torch

import loudness_reference as lr
import synth_reference as sr_
from bsed_amd.labels import BIRD_LIST, ManyHotEncoder

pytestmark = pytest.mark.gpu

SR = 32000
N_CLIP = 2 * SR
_cache = {}


def bank_items(sr=SR):
    """events [(label, waveform)] and backgrounds: a high chirp, a low rumble, noise, a click shorter than a block, a PCM16
    snippet, a silent snippet; a background of exactly one clip, a shorter one and a silent one"""
    rng = np.random.default_rng(21)
    t = lambda n: np.arange(n) / sr
    chirp = 0.3 * np.sin(2 * np.pi * (3000.0 + 2500.0 * t(24000)) * t(24000))
    rumble = 0.4 * np.sin(2 * np.pi * 60.0 * t(40000)) + 0.01 * rng.standard_normal(40000)
    half_silent = np.concatenate([0.2 * rng.standard_normal(9000), np.zeros(9000)])
    events = [(BIRD_LIST[0], chirp.astype(np.float32)), (BIRD_LIST[1], rumble.astype(np.float32)),
              (BIRD_LIST[2], half_silent.astype(np.float32)), (BIRD_LIST[3], (0.5 * rng.standard_normal(801)).astype(np.float32)),
              (BIRD_LIST[4], rng.integers(-9000, 9000, size=12000).astype(np.int16)),
              (BIRD_LIST[2], np.zeros(5000, np.float32))]
    wind = 0.05 * np.cumsum(rng.standard_normal(N_CLIP)) / 30.0 + 0.02 * rng.standard_normal(N_CLIP)
    backgrounds = [wind.astype(np.float32), (0.03 * rng.standard_normal(50001)).astype(np.float32), np.zeros(7000, np.float32)]
    return events, backgrounds


def _as_f32(w):
    return w if w.dtype == np.float32 else w.astype(np.float32) * np.float32(1.0 / 32768.0)


def _banks():
    if "banks" not in _cache:
        from bsed_amd import synth
        events, backgrounds = bank_items()
        _cache["banks"] = (synth.SoundBank(events, backgrounds, BIRD_LIST, SR, loudness="lufs"),
                           synth.SoundBank(events, backgrounds, BIRD_LIST, SR))
    return _cache["banks"]


def test_bank_measures_every_item_in_lufs_and_keeps_its_rms():
    bank, plain = _banks()
    events, backgrounds = bank_items()
    assert plain.lufs is None and bank.lufs.dtype == np.float64 and bank.lufs.shape == (9,)
    assert np.array_equal(bank.rms, plain.rms) and torch.equal(bank.flat, plain.flat)
    worst = 0.0
    for k, w in enumerate([w for _, w in events] + backgrounds):
        loud, _, margin = lr.loudness_of(_as_f32(w), SR)
        lr.assert_decidable(margin, f"item {k}")
        if math.isinf(loud):
            assert bank.lufs[k] == loud and k in (5, 8)
        else:
            worst = max(worst, abs(bank.lufs[k] - loud))
            assert abs(bank.lufs[k] - loud) <= lr.BAR, (k, bank.lufs[k], loud)
    print(f"bank: worst |lufs - ref| = {worst:.3e} LU; lufs = {np.round(bank.lufs, 3).tolist()}")
    # what the K-weighting and the gate change against plain RMS: the 60 Hz rumble reads lower than its RMS level, the
    # chirp at 3-5.5 kHz higher, the half-silent snippet as its loud half
    rms_db = 20.0 * np.log10(bank.rms[:3])
    assert bank.lufs[1] - rms_db[1] < -2.5 and bank.lufs[0] - rms_db[0] > 1.5 and bank.lufs[2] - rms_db[2] > 2.0


def test_a_clip_that_is_one_whole_background_measures_ref_db():
    """bg_len == n and phase 0: the clip is the background times one float32 gain, so it measures ref_db but for the
    rounding of that gain (2^-24 relative: 5e-7 dB) and of the products"""
    from bsed_amd import features, synth
    bank, _ = _banks()
    assert bank.length[6] == N_CLIP
    plan = synth.plan_soundscapes(bank, 6, np.random.default_rng(3), n_samples=N_CLIP, n_events=(0, 0), ref_db=-30.0,
                                  loudness="lufs")
    plan.bg_phase[:] = 0
    plan.validate(bank)
    whole = np.nonzero(plan.bg_len == N_CLIP)[0]
    assert len(whole) >= 1 and (plan.n_ev == 0).all()
    loud = features.loudness(synth.mix(bank, plan), SR).cpu().numpy()
    assert np.abs(loud[whole] - (-30.0)).max() <= 1e-5, loud
    silent = np.nonzero(plan.bg_len == 7000)[0]
    assert (plan.bg_gain[silent] == 0).all() and (loud[silent] == -math.inf).all()


SEED = 2023


def lufs_batch_plan(bank, seed=SEED):
    from bsed_amd import synth
    enc = ManyHotEncoder(BIRD_LIST, n_frames=N_CLIP // 255 // 4, sr=SR)
    syn = synth.Synthesizer(bank, enc, N_CLIP, seed=seed, n_events=(2, 5), ref_db=-40.0, snr_db=(6.0, 30.0), loudness="lufs")
    return syn, syn.plan(4, 0)


def test_synthesized_batch_has_the_loudness_of_the_float64_mix_of_its_plan():
    from bsed_amd import features
    bank, _ = _banks()
    syn, plan = lufs_batch_plan(bank)
    waves, strong, weak, plan2 = syn.batch(4, 0)
    assert np.array_equal(plan.g, plan2.g) and (plan.n_ev >= 2).all() and (plan.bg_len > 0).all()
    ref, _, _ = sr_.mix_ref(bank.flat.cpu().numpy(), plan)
    got = features.loudness(waves, SR).cpu().numpy()
    checked = 0
    for b in range(4):
        loud, _, margin = lr.loudness_of(ref[b], SR)
        if margin <= lr.MARGIN:
            continue
        checked += 1
        assert abs(got[b] - loud) <= 1e-5, (b, got[b], loud)
    assert checked >= 3
    print(f"batch: loudness {np.round(got, 3).tolist()}, {checked} of 4 clips decidable")
