"""Soundscape synthesis on the device (csrc/synth.hip, bsed_amd.synth): the mix against the float64 reference of
tests/synth_reference.py within its fp32 bound, its independence of the launch partition, the targets against the
encoder's own rasterisation, the bank against ``features.load_audio``, and batches through a train step and through the
on-disk format.

Shapes: n = 20011 samples (prime: a ragged last tile, rows of the output off the 16-byte grid), B = 3; the kernel's tile
is 4096 samples, below the 6000 at which the clip would have to grow to keep three tiles."""
import os
import wave

import numpy as np
import pytest
import torch

import synth_reference as sr_
from bsed_amd.labels import BIRD_LIST, ManyHotEncoder

pytestmark = pytest.mark.gpu

_cache = {}


def _bank():
    """the seven-item bank of synth_reference (built once): (SoundBank, its samples as one float32 numpy array)"""
    if "bank" not in _cache:
        from bsed_amd import synth
        items = sr_.hand_bank_samples()
        ev = [(BIRD_LIST[c], w) for w, c in zip(items, sr_.ITEM_CLASS) if c >= 0]
        bank = synth.SoundBank(ev, [w for w, c in zip(items, sr_.ITEM_CLASS) if c < 0], BIRD_LIST)
        _cache["bank"] = (bank, np.concatenate(items))
    return _cache["bank"]


def _mixed():
    """the hand-built plan, its mix on the device and the float64 reference (computed once, never modified)"""
    if "mixed" not in _cache:
        from bsed_amd import synth
        bank, flat = _bank()
        plan = sr_.hand_plan(synth, BIRD_LIST).validate(bank)
        out = synth.mix(bank, plan)
        _cache["mixed"] = (plan, out, sr_.mix_ref(flat, plan))
    return _cache["mixed"]


def test_bank_holds_the_items_back_to_back():
    bank, flat = _bank()
    assert bank.offset.tolist() == sr_.ITEM_OFF.tolist() and bank.length.tolist() == sr_.ITEM_LEN
    assert bank.cls.tolist() == sr_.ITEM_CLASS and bank.backgrounds.tolist() == [5, 6]
    assert np.array_equal(bank.flat.cpu().numpy(), flat)
    assert bank.items(BIRD_LIST[2]).tolist() == [2, 4] and bank.items(BIRD_LIST[9]).tolist() == []
    items = sr_.hand_bank_samples()
    want = np.array([np.sqrt(np.mean(w.astype(np.float64) ** 2)) for w in items])
    np.testing.assert_allclose(bank.rms, want, rtol=1e-12)


def test_mix_is_within_the_fp32_bound_of_the_float64_reference():
    """worst |err| / bound measured on MI355X: see DESIGN.md, "Soundscape synthesis" """
    plan, out, (ref, S, K) = _mixed()
    assert plan.n_ev.tolist() == [7, 0, 16] and plan.bg_len.tolist() == [997, 25000, 0]
    assert K[2].max() == 8 and K[0, 3001:4001].min() == 3         # eight deep in clip 2; two events + the long one in clip 0
    got = out.cpu().numpy().astype(np.float64)
    assert got.shape == (3, sr_.N_HAND)
    bound = (2 * K + 2) * sr_.U24 * S
    err = np.abs(got - ref)
    silent = S == 0
    assert silent[2].any() and (got[silent] == 0).all()            # silence where nothing plays: exact zeros, all written
    ratio = (err[~silent] / bound[~silent]).max()
    print(f"synth_mix: worst |err| / bound = {ratio:.4f}; worst |err| = {err.max():.3e}; largest |ref| = {np.abs(ref).max():.3e}")
    assert (err <= bound).all(), ratio
    # the one-sample event and the background's wrap, spelled out
    bank, flat = _bank()
    assert got[1, 0] == np.float64(flat[sr_.ITEM_OFF[6] + 24999]) and got[1, 1] == np.float64(flat[sr_.ITEM_OFF[6]])


def test_mix_is_repeatable_and_independent_of_the_partition():
    from bsed_amd import synth
    bank, _ = _bank()
    plan, out, _ = _mixed()
    assert torch.equal(synth.mix(bank, plan), out)                 # a second launch: the same bits
    rows = sr_.hand_rows()
    for b in range(3):                                             # clip b alone (B = 1; its row starts 16-byte aligned)
        alone = synth.mix(bank, sr_.hand_plan(synth, BIRD_LIST, rows=[rows[b]]).validate(bank))
        assert torch.equal(alone[0], out[b]), b
    two = sr_.hand_plan(synth, BIRD_LIST, rows=rows[:2]).validate(bank)        # largest n_ev = 7
    assert torch.equal(synth.mix(bank, two), out[:2])
    assert torch.equal(synth.mix(bank, two, K=7), out[:2])         # K = 16 with unused slots == K = the largest n_ev
    tight = sr_.hand_plan(synth, BIRD_LIST, rows=rows[:2], K=7).validate(bank)
    assert torch.equal(synth.mix(bank, tight), out[:2])


def test_mix_indexes_a_bank_and_an_output_past_2_to_the_31_elements():
    """64-bit positions: a snippet that starts past sample 2^31 of the bank, written into a row that starts past element
    2^31 of the output (3 clips of 2^30 + 3 samples: 12.9 GB written once, ~2 ms; only the touched ends are read back)"""
    from bsed_amd import synth
    big, n, ln = 2 ** 31 + 5000, 2 ** 30 + 3, 1000
    bank = synth.SoundBank.layout(BIRD_LIST, [big], [0], [1.0])
    bank.flat = torch.empty(big, device="cuda", dtype=torch.float32)            # uninitialised but for the snippet
    snippet = torch.randn(ln, device="cuda", generator=torch.Generator(device="cuda").manual_seed(2))
    src = 2 ** 31 + 101
    bank.flat[src:src + ln] = snippet
    z = np.zeros((3, 1))
    on = np.array([[0], [0], [n - ln]])
    plan = synth.SoundscapePlan(n, 32000, BIRD_LIST, [0] * 3, [0] * 3, [0] * 3, [0.0] * 3, [0, 0, 1], z + src, on, z + ln,
                                z + 1, z + 1, z).validate(bank)                  # gain 1, no fade: the samples themselves
    out = synth.mix(bank, plan)
    assert out.shape == (3, n) and 2 * n + (n - ln) > 2 ** 31
    assert torch.equal(out[2, n - ln:], snippet)
    assert (out[2, n - ln - 4096:n - ln] == 0).all() and (out[2, :4096] == 0).all()
    assert (out[0, :4096] == 0).all() and (out[1, n - 4096:] == 0).all()
    del out, bank


def _boundary_plan(synth, sr):
    """two clips of 11 s around the onsets at which integer division gives another frame: events of one class that
    overlap, and events that run past frame T' of a 10 s encoder"""
    n = 11 * sr
    ons = [s + d for s in sr_.BOUNDARY_ONSETS[sr] for d in (-1, 0, 1)]
    K = 16
    P = dict(n_ev=[len(ons), 4], src=np.zeros((2, K)), on=np.zeros((2, K)), length=np.ones((2, K)), g=np.ones((2, K)),
             inv_fade=np.ones((2, K)), cls=np.zeros((2, K)))
    for k, s in enumerate(ons):
        P["on"][0, k], P["length"][0, k], P["cls"][0, k] = s, 1021 + 300 * k, k % 3        # neighbours of a class overlap
    last = [(10 * sr - 4000, 3000, 5), (10 * sr - 2000, sr, 5), (10 * sr + 2000, 500, 6), (0, n, 7)]   # past T', beyond T', all
    for k, (s, ln, c) in enumerate(last):
        P["on"][1, k], P["length"][1, k], P["cls"][1, k] = s, ln, c
    return synth.SoundscapePlan(n, sr, BIRD_LIST, [0, 0], [0, 0], [0, 0], [0.0, 0.0], **P)


@pytest.mark.parametrize("sr,n_frames", [(32000, 313), (22050, 216)])
def test_targets_are_the_encoders_rasterisation_of_the_annotations(sr, n_frames):
    from bsed_amd import synth
    enc = ManyHotEncoder(BIRD_LIST, n_frames=n_frames, sr=sr)
    for plan in (sr_.hand_plan(synth, BIRD_LIST, sr=sr), _boundary_plan(synth, sr)):
        strong, weak = synth.targets(plan, n_frames)
        assert strong.shape == (plan.B, n_frames, len(BIRD_LIST)) and weak.shape == (plan.B, len(BIRD_LIST))
        for merge in (True, False):
            ann = plan.annotations(merge_same_label=merge)
            for b in range(plan.B):
                want = enc.encode_strong_df(ann[ann["filename"] == plan.names[b] + ".wav"])
                assert np.array_equal(strong[b].cpu().numpy(), want.astype(np.float32)), (sr, b, merge)
        assert torch.equal(weak, strong.max(1)[0])
        assert strong.sum() > 0
    assert strong[1, -1, 5] == 1 and strong[1, -1, 7] == 1 and strong[1, :, 6].sum() == 0      # clipped at T'; beyond it


def _write_wav(path, x, sr):
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with wave.open(path, "wb") as f:
        f.setnchannels(x.shape[1])
        f.setsampwidth(2)
        f.setframerate(sr)
        f.writeframes(np.ascontiguousarray(x, dtype="<i2").tobytes())


def test_bank_from_folders_holds_load_audios_samples(tmp_path):
    from bsed_amd import synth
    from bsed_amd._lib import BsedError
    from bsed_amd.features import load_audio
    rng = np.random.default_rng(3)
    files = [("fg/EATO/a.wav", 44100, 2, 3000), ("fg/WOTH/b.wav", 32000, 1, 2001), ("bg/site/c.wav", 22050, 1, 1500)]
    for rel, sr, ch, nfr in files:
        _write_wav(str(tmp_path / rel), rng.integers(-20000, 20000, size=(nfr, ch)).astype(np.int16), sr)
    bank = synth.SoundBank.from_folders(str(tmp_path / "fg"), str(tmp_path / "bg"), BIRD_LIST, sr=32000)
    assert len(bank) == 3 and bank.cls.tolist() == [BIRD_LIST.index("EATO"), BIRD_LIST.index("WOTH"), -1]
    for item, (rel, *_) in enumerate(files):
        want, sr = load_audio(str(tmp_path / rel), 32000)
        assert sr == 32000 and torch.equal(bank.wave(item), want), rel
        x = want.cpu().numpy().astype(np.float64)
        assert abs(bank.rms[item] - np.sqrt(np.mean(x * x))) <= 1e-12 * np.sqrt(np.mean(x * x))
    assert bank.total_samples == int(bank.flat.numel()) == int(bank.length.sum())
    with pytest.raises(BsedError):
        synth.SoundBank.from_folders(str(tmp_path / "fg"), None, ["EATO"], sr=32000)         # WOTH/ is not a label
    with pytest.raises(BsedError):
        synth.SoundBank([("EATO", np.zeros(0, np.float32))], [], BIRD_LIST)                 # an empty snippet
    with pytest.raises(BsedError):
        synth.SoundBank([("XXXX", np.zeros(10, np.float32))], [], BIRD_LIST)                # a label outside the list


N_E2E = 8160          # 33 mel frames, T' = 8


def _synthesizer(seed=2023):
    from bsed_amd import synth
    if "e2e_bank" not in _cache:
        rng = np.random.default_rng(8)
        ev = [(BIRD_LIST[k % 5], (0.2 * rng.standard_normal(ln)).astype(np.float32))
              for k, ln in enumerate([700, 1500, 3001, 6400, 8160, 12000])]
        ev.append((BIRD_LIST[5], rng.integers(-9000, 9000, size=2500).astype(np.int16)))      # PCM16 snippets are taken too
        _cache["e2e_bank"] = synth.SoundBank(ev, [(0.05 * rng.standard_normal(20000)).astype(np.float32)], BIRD_LIST)
    enc = ManyHotEncoder(BIRD_LIST, n_frames=N_E2E // 255 // 4, sr=32000)
    return synth.Synthesizer(_cache["e2e_bank"], enc, N_E2E, seed=seed, n_events=(1, 4))


def test_batches_feed_the_train_step_and_the_prefetch_changes_nothing():
    from oracle import crnn_oracle as co
    from bsed_amd.engine import FlatAdam, SEDTrainer
    from bsed_amd.features import MelConfig, MelFrontEnd
    from bsed_amd.models import CRNN, Predictor, weights_init
    syn = _synthesizer()
    w, y, weak, plan = syn.batch(2, 0)
    assert w.shape == (2, N_E2E) and y.shape == (2, 8, 20) and weak.shape == (2, 20) and plan.B == 2
    assert torch.isfinite(w).all() and w.abs().max() > 0 and y.sum() > 0
    w_again = syn.batch(2, 0)[0]
    assert torch.equal(w, w_again) and not torch.equal(w, syn.batch(2, 1)[0])      # a step repeats; steps differ
    fe = MelFrontEnd(MelConfig())
    runs = []
    for prefetch in (False, True):
        torch.manual_seed(0)
        crnn, pred = CRNN(**co.CRNN_KWARGS), Predictor(**co.PREDICTOR_KWARGS)
        weights_init(crnn); weights_init(pred)
        tr = SEDTrainer(crnn, pred, optimizer=FlatAdam([crnn, pred], lr=1e-3), frontend=fe, seed=4)
        w0, y0, *_ = syn.batch(2, 0)
        losses = []
        for k in range(2):
            w1, y1, *_ = syn.batch(2, k + 1)
            out = tr.train_step(w0, y0, from_wave=True, next_waves=(w1, None) if prefetch else None)
            losses.append(SEDTrainer.loss_value(out))
            w0, y0 = w1, y1
        assert np.isfinite(losses).all()
        runs.append((losses, crnn.flat.clone(), pred.flat.clone()))
    assert runs[0][0] == runs[1][0]
    assert torch.equal(runs[0][1], runs[1][1]) and torch.equal(runs[0][2], runs[1][2])


def test_write_dataset_round_trips_through_the_feature_dataset(tmp_path):
    from bsed_amd.data import FeatureDataset
    from bsed_amd.features import preprocess
    syn = _synthesizer(seed=9)
    names = syn.write_dataset(str(tmp_path), 3, B=3)
    assert names == ["syn_00000", "syn_00001", "syn_00002"]
    waves, strong, _, plan = syn.batch(3, 0)
    ds = FeatureDataset(str(tmp_path), syn.encoder.encode_strong_df)
    assert len(ds) == 3
    for b in range(3):
        (mel, target), path = ds[b]
        assert os.path.basename(path) == names[b] + ".npy"
        assert np.array_equal(mel, preprocess(waves[b].cpu().numpy()))
        assert np.array_equal(target.astype(np.float32), strong[b].cpu().numpy())
        assert target.sum() > 0
