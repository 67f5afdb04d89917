"""Dataset scaler on the GPU: the statistics kernels (csrc/scaler.hip), the normalised dB kernels (csrc/mel.hip) and
their wiring into the front end, the collate function, the trainer and a captured step.

Every reference is made from the GPU's own UNNORMALISED ``to_db`` / ``transform`` output (a front end without a scaler),
copied to the host and put through tests/scaler_reference.py, so that only the new code is under test:

  statistics     mean_ and mean_of_square_ within rtol 1e-12 of the restatement (float32 square, float64 sums).  Only the
                 order of the float64 additions differs: at most 1500 terms per band here, error near 2e-13 at worst.
                 A float64 square (5e-9 away), or a dB value that is not bitwise ``to_db``'s, fails.
  normalisation  bitwise ``float32((float64(to_db) - mean_) / std_)``: a float64 division is correctly rounded and the
                 build has no fast-math flag, so there is no tolerance."""
import os

import numpy as np
import pytest
import torch

import scaler_reference as sref
from conftest import GOLDEN
from oracle import seeded

pytestmark = pytest.mark.gpu

RTOL = 1e-12
T_IN = 37


@pytest.fixture(scope="module")
def fes():
    """front ends WITHOUT a scaler, per n_mels: the source of every reference (40 bands up to 4 kHz: the STFT kernel's
    filterbank table holds no 40 bands as wide as those up to 16 kHz; the kernels under test never see the filters)"""
    from bsed_amd.features import MelConfig, MelFrontEnd
    return {128: MelFrontEnd(MelConfig(n_mels=128)), 40: MelFrontEnd(MelConfig(n_mels=40, mel_f_max=4000.0))}


def _linear(seed, B, T, M, zero_clip=None):
    """random positive linear mel over ~6 decades (so that the per-clip top_db floor clamps part of it), some exact
    zeros, optionally one all-zero clip"""
    rng = np.random.RandomState(seed)
    x = np.exp(rng.normal(-4.0, 3.0, size=(B, T, M))).astype(np.float32)
    x[rng.uniform(size=x.shape) < 0.02] = 0.0
    if zero_clip is not None:
        x[zero_clip] = 0.0
    return torch.from_numpy(x).cuda()


def _batches(M, T=T_IN):
    """the issue's pair of updates: B = 3 (one all-zero clip) followed by B = 2"""
    return [_linear(11 + M, 3, T, M, zero_clip=1), _linear(12 + M, 2, T, M)]


def _db(fe, mel, T_out):
    cmax, _ = fe.stats(mel)
    return fe.to_db(mel, cmax, T_out)


def _ref_stats(fe, mels, T_out):
    assert fe.scaler is None
    x = np.concatenate([_db(fe, m, T_out).cpu().numpy() for m in mels])
    return sref.statistics(x)


def _check_stats(s, ref, what=""):
    mean, msq = ref
    np.testing.assert_allclose(s.mean_, mean, rtol=RTOL, atol=0, err_msg=f"{what} mean_")
    np.testing.assert_allclose(s.mean_of_square_, msq, rtol=RTOL, atol=0, err_msg=f"{what} mean_of_square_")
    np.testing.assert_array_equal(s.std_, sref.std_of(s.mean_, s.mean_of_square_))
    assert s.mean_.dtype == s.std_.dtype == np.float64 and s.mean_.shape == s.std_.shape == mean.shape


def _scaler_of(fe, mels, T_out):
    from bsed_amd.scaler import Scaler
    s = Scaler()
    for m in mels:
        s.update(m, max_frames=T_out, top_db=fe.cfg.top_db)
    s.finish()
    return s


def _golden_scaler():
    from bsed_amd.scaler import Scaler
    return Scaler().load(os.path.join(GOLDEN, "scaler_state.json"))


def _same_bits(got, want, what=""):
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else got
    assert got.dtype == np.float32 and got.shape == want.shape, (what, got.dtype, got.shape, want.shape)
    bad = got.view(np.uint32) != want.view(np.uint32)
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} elements differ"


# ----------------------------------------------------------------------------------------------------------------------
# statistics
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T_out", [29, 37, 50])
@pytest.mark.parametrize("M", [128, 40])
def test_statistics_from_linear_mel(fes, M, T_out):
    from bsed_amd.scaler import Scaler
    fe, mels = fes[M], _batches(M)
    s = Scaler()
    cmax, _ = fe.stats(mels[0])
    s.update(mels[0], cmax, max_frames=T_out, top_db=fe.cfg.top_db)
    s.update(mels[1], max_frames=T_out, top_db=fe.cfg.top_db)          # clip_max absent: computed as MelFrontEnd.stats does
    mean, std = s.finish()
    assert mean is s.mean_ and std is s.std_
    _check_stats(s, _ref_stats(fe, mels, T_out), f"M{M} T_out{T_out}")


@pytest.mark.parametrize("M", [128, 40])
def test_statistics_over_several_row_chunks_with_a_ragged_tail(fes, M):
    """T = T_out = 300: five chunks of 64 rows per clip, the last with 44"""
    fe, mels = fes[M], _batches(M, T=300)
    _check_stats(_scaler_of(fe, mels, 300), _ref_stats(fe, mels, 300), f"M{M} T300")


def test_statistics_from_unaligned_linear_mel_take_the_scalar_loads(fes):
    """n_mels = 128 at an address that is no multiple of 16 bytes: no float4 loads there"""
    fe, mels = fes[128], _batches(128)
    shifted = []
    for m in mels:
        buf = torch.empty(m.numel() + 1, device="cuda", dtype=torch.float32)
        v = buf[1:].view(m.shape)
        v.copy_(m)
        assert v.data_ptr() % 16 == 4 and v.is_contiguous()
        shifted.append(v)
    _check_stats(_scaler_of(fe, shifted, 50), _ref_stats(fe, mels, 50), "unaligned")


@pytest.mark.parametrize("M", [128, 40])
def test_statistics_from_a_db_tensor(fes, M):
    from bsed_amd.scaler import Scaler
    fe, mels = fes[M], _batches(M)
    s = Scaler()
    for m in mels:
        s.update_db(_db(fe, m, 50))
    s.finish()
    _check_stats(s, _ref_stats(fe, mels, 50), f"db M{M}")


def test_statistics_from_waveforms(fes):
    from bsed_amd.scaler import Scaler
    fe = fes[128]
    n = 255 * 36
    assert fe.num_frames(n) == T_IN
    g = torch.Generator(device="cuda").manual_seed(3)
    wavs = [torch.randn(B, n, device="cuda", generator=g) * 0.1 for B in (3, 2)]
    s = Scaler()
    for w in wavs:
        s.update_waves(w, fe, max_frames=50)
    s.finish()
    x = np.concatenate([fe.transform(w, max_frames=50).cpu().numpy() for w in wavs])
    _check_stats(s, sref.statistics(x), "waves")


def test_same_updates_give_the_same_bits_and_merge_equals_one_pass(fes):
    from bsed_amd.scaler import Scaler
    fe, mels = fes[128], _batches(128, T=300)
    one, two = _scaler_of(fe, mels, 300), _scaler_of(fe, mels, 300)
    assert torch.equal(one._acc, two._acc)
    np.testing.assert_array_equal(one.mean_, two.mean_)
    np.testing.assert_array_equal(one.mean_of_square_, two.mean_of_square_)
    a, b = Scaler().update(mels[0]), Scaler().update(mels[1])
    a.merge(b)
    a.finish()
    _check_stats(a, _ref_stats(fe, mels, 300), "merge")
    from bsed_amd import _lib as L
    with pytest.raises(L.BsedError, match="shapes differ"):
        a.merge(Scaler().update(mels[0], max_frames=29))


def test_calculate_scaler_takes_both_kinds_of_dataset(fes):
    from bsed_amd.scaler import Scaler
    fe = fes[128]
    mels = _batches(128)
    # the reference's transformed data set: ((dB tensor (1, T, n_mels), target), path)
    db = np.concatenate([_db(fe, m, 50).cpu().numpy() for m in mels])
    items = [((torch.from_numpy(c), np.zeros(3, dtype=np.float32)), f"clip{i}") for i, c in enumerate(db)]
    s = Scaler()
    mean, std = s.calculate_scaler(items, batch=2)
    _check_stats(s, sref.statistics(db), "dB data set")
    # FeatureDataset(transform=None): linear mel of two lengths, each clip with its own clamp, (features, target) items
    lin = [m.cpu().numpy() for m in (_linear(31, 3, T_IN, 128), _linear(32, 2, 30, 128))]
    items = [(c, np.zeros(3, dtype=np.float32)) for group in lin for c in group]
    s = Scaler()
    s.calculate_scaler(items, frontend=fe, max_frames=40, batch=2)
    want = np.concatenate([_db(fe, torch.from_numpy(g).cuda(), 40).cpu().numpy() for g in lin])
    _check_stats(s, sref.statistics(want), "linear data set")


# ----------------------------------------------------------------------------------------------------------------------
# normalisation
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T_out", [29, 37, 50])
@pytest.mark.parametrize("M", [128, 40])
def test_normalised_to_db_is_bitwise_the_formula(fes, M, T_out):
    from bsed_amd.features import MelFrontEnd
    fe, mels = fes[M], _batches(M)
    s = _scaler_of(fe, mels, T_out)
    fe_s = MelFrontEnd(fe.cfg, scaler=s)
    assert fe_s.scaler is s
    for k, m in enumerate(mels):
        cmax, _ = fe.stats(m)
        plain = fe.to_db(m, cmax, T_out).cpu().numpy()
        got = fe_s.to_db(m, cmax, T_out)
        assert got.shape == (m.shape[0], 1, T_out, M)
        _same_bits(got, sref.normalize(plain, s.mean_, s.std_), f"M{M} T_out{T_out} batch {k}")
        if T_out > T_IN:
            pad = np.broadcast_to((-s.mean_ / s.std_).astype(np.float32), (m.shape[0], 1, T_out - T_IN, M))
            _same_bits(got[:, :, T_IN:].contiguous(), np.ascontiguousarray(pad), "pad rows")
    # detaching restores the unnormalised kernel
    fe_s.set_scaler(None)
    cmax, _ = fe.stats(mels[0])
    assert torch.equal(fe_s.to_db(mels[0], cmax, T_out), fe.to_db(mels[0], cmax, T_out))


def test_normalised_to_db_over_many_rows(fes):
    from bsed_amd.features import MelFrontEnd
    fe, mels = fes[128], _batches(128, T=300)
    s = _golden_scaler()
    fe_s = MelFrontEnd(fe.cfg, scaler=s)
    cmax, _ = fe.stats(mels[0])
    _same_bits(fe_s.to_db(mels[0], cmax, 300), sref.normalize(fe.to_db(mels[0], cmax, 300).cpu().numpy(), s.mean_, s.std_), "T300")


@pytest.mark.parametrize("T_out", [29, 37, 50])
def test_normalised_views_are_the_normalised_tensor_and_its_rolls(fes, T_out):
    from bsed_amd.features import MelFrontEnd
    fe, m = fes[128], _batches(128)[0]
    s = _golden_scaler()
    fe_s = MelFrontEnd(fe.cfg, scaler=s)
    cmax, _ = fe.stats(m)
    want = torch.from_numpy(sref.normalize(fe.to_db(m, cmax, T_out).cpu().numpy(), s.mean_, s.std_)).cuda()
    sh, sw = [-3, T_out + 24, 0], [130, -5, 7]       # negative, beyond T_out, beyond 128
    x, xt, xf = fe_s.to_db_views(m, cmax, sh, sw, T_out)
    assert torch.equal(x, want)
    for b in range(3):
        assert torch.equal(xt[b], torch.roll(want[b], sh[b], dims=-2)), ("time", b)
        assert torch.equal(xf[b], torch.roll(want[b], sw[b], dims=-1)), ("frequency", b)


def test_transform_normalises_both_members_of_the_pair(fes):
    from bsed_amd.features import MelFrontEnd
    fe = fes[128]
    s = _golden_scaler()
    fe_s = MelFrontEnd(fe.cfg, scaler=s)
    n = 255 * 36
    g = torch.Generator(device="cuda").manual_seed(4)
    wav = torch.randn(3, n, device="cuda", generator=g) * 0.1
    unit = torch.randn(3, T_IN, 128, device="cuda", generator=g)
    clean, noisy = fe.transform(wav, max_frames=50, noisy=True, unit_noise=unit)
    assert not torch.equal(clean, noisy)
    got_c, got_n = fe_s.transform(wav, max_frames=50, noisy=True, unit_noise=unit)
    _same_bits(got_c, sref.normalize(clean.cpu().numpy(), s.mean_, s.std_), "clean")
    _same_bits(got_n, sref.normalize(noisy.cpu().numpy(), s.mean_, s.std_), "noisy")
    # and the triple of views, through transform
    got = fe_s.transform(wav, max_frames=50, views=([5, -7, 60], [3, 200, -1]))
    assert torch.equal(got[0], got_c) and torch.equal(got[1][1], torch.roll(got_c[1], -7, dims=-2))
    assert torch.equal(got[2][1], torch.roll(got_c[1], 200, dims=-1))


def test_gpu_collate_follows_the_front_end(fes):
    from bsed_amd.data import GpuCollate
    from bsed_amd.features import MelFrontEnd
    fe = fes[128]
    s = _golden_scaler()
    fe_s = MelFrontEnd(fe.cfg, scaler=s)
    a, b = _linear(41, 2, T_IN, 128).cpu().numpy(), _linear(42, 1, 30, 128).cpu().numpy()
    b[0] *= 1e-3                                     # another clip max: its own clamp
    items = [((a[0], np.ones(4, dtype=np.float32)), "a0"), ((b[0], np.zeros(4, dtype=np.float32)), "b0"),
             ((a[1], np.ones(4, dtype=np.float32)), "a1")]
    ((pc, pn), pt), pp = GpuCollate(fe, max_frames=40, noisy=True, seed=7)(items)
    ((gc_, gn), gt), gp = GpuCollate(fe_s, max_frames=40, noisy=True, seed=7)(items)
    assert gp == pp == ["a0", "b0", "a1"] and torch.equal(gt, pt) and gc_.shape == (3, 1, 40, 128)
    _same_bits(gc_, sref.normalize(pc.cpu().numpy(), s.mean_, s.std_), "clean")
    _same_bits(gn, sref.normalize(pn.cpu().numpy(), s.mean_, s.std_), "noisy")
    assert float(pc[1].min()) < float(pc[0].min()) - 20.0       # the quiet clip kept its own floor


def test_scaler_normalize_on_a_gpu_tensor(fes):
    fe, m = fes[40], _batches(40)[0]
    s = _scaler_of(fe, [m], 50)
    x = _db(fe, m, 50)
    got = s.normalize(x)
    assert got.is_cuda and got.shape == x.shape
    _same_bits(got, sref.normalize(x.cpu().numpy(), s.mean_, s.std_), "normalize")
    assert torch.equal(s.normalize(x.cpu()).cuda(), got)


def test_attaching_unusable_statistics_raises(fes):
    from bsed_amd import _lib as L
    from bsed_amd.features import MelFrontEnd
    from bsed_amd.scaler import Scaler
    fe = fes[128]
    with pytest.raises(L.BsedError, match="no statistics"):
        MelFrontEnd(fe.cfg, scaler=Scaler())
    s = _golden_scaler()
    s.std_[5] = 0.0
    with pytest.raises(L.BsedError, match="5"):
        MelFrontEnd(fe.cfg).set_scaler(s)
    with pytest.raises(L.BsedError, match="128 bands"):
        MelFrontEnd(fes[40].cfg, scaler=_golden_scaler())
    # bands that never vary (-8 dB: sums and squares are exact, the variance is exactly 0): finish names them
    flat = torch.full((2, 1, 10, 40), -8.0, device="cuda")
    with pytest.raises(L.BsedError, match=r"band\(s\) \[0, 1, 2"):
        Scaler().update_db(flat).finish()


# ----------------------------------------------------------------------------------------------------------------------
# trainer, checkpoint, captured step
# ----------------------------------------------------------------------------------------------------------------------
B0, T0 = 4, 128


def _waves(k, seed=5):
    from bsed_amd.features import MelConfig
    n = 127 * MelConfig().hop_size
    g = torch.Generator(device="cuda").manual_seed(seed)
    return [(torch.randn(B0, n, device="cuda", generator=g) * 0.1,
             torch.from_numpy(seeded.strong_targets(90 + i, B0, T0 // 4)).cuda()) for i in range(k)]


def test_train_step_from_waves_equals_the_step_fed_normalised_features(fes):
    """The smallest CRNN configuration of the trainer tests, dropout off.  The two inputs are bitwise equal (asserted
    here once more), so the steps may differ only as much as two runs of the feature-fed step from the same state differ
    from each other: that is measured here, and is the bound (bitwise where they are bitwise)."""
    from bsed_amd import checkpoint
    from bsed_amd.engine import FlatAdam, SEDTrainer
    from bsed_amd.features import MelFrontEnd
    from oracle import crnn_oracle as co
    from test_crnn_gpu import _mine, _oracle
    fe = fes[128]
    s = _golden_scaler()
    fe_s = MelFrontEnd(fe.cfg, scaler=s)
    data = _waves(2)
    feats = [s.normalize(fe.transform(w, max_frames=T0)) for w, _ in data]
    for (w, _), x in zip(data, feats):
        assert fe.num_frames(w.shape[1]) == T0 and torch.equal(fe_s.transform(w, max_frames=T0), x)
    ocrnn, opred = _oracle(0.0, 9)

    def run(kind):
        crnn, pred = _mine(0.0, ocrnn, opred)
        tr = SEDTrainer(crnn, pred, optimizer=FlatAdam([crnn, pred], lr=1e-3), frontend=fe_s if kind == "wave" else None,
                        seed=11)
        losses = []
        for (w, y), x in zip(data, feats):
            out = tr.train_step(w, y, from_wave=True) if kind == "wave" else tr.train_step(x, y)
            losses.append(SEDTrainer.loss_value(out))
        torch.cuda.synchronize()
        return losses, [crnn.flat.clone(), pred.flat.clone(), crnn.flat_buf.clone()], (crnn, pred)

    la, ta, _ = run("features")
    lb, tb, _ = run("features")
    lw, tw, (crnn, pred) = run("wave")
    spread_loss = max(abs(a - b) for a, b in zip(la, lb))
    spread = [float((a - b).abs().max()) for a, b in zip(ta, tb)]
    got_loss = max(abs(a - b) for a, b in zip(la, lw))
    got = [float((a - b).abs().max()) for a, b in zip(ta, tw)]
    print(f"feature-fed twice: loss {spread_loss:g}, weights {spread}; wave-fed against it: loss {got_loss:g}, weights {got}")
    assert all(np.isfinite(l) for l in lw)
    assert got_loss <= spread_loss, (got_loss, spread_loss)
    for g, sp in zip(got, spread):
        assert g <= sp, (got, spread)
    # the checkpoint carries the scaler and load_models rebuilds it
    kw = dict(co.CRNN_KWARGS)
    kw["dropout"] = 0.0
    st = checkpoint.build_state(crnn, pred, kw, dict(co.PREDICTOR_KWARGS), scaler=s)
    back = checkpoint.load_models(st)
    assert isinstance(back["scaler"], type(s))
    for name in ("mean_", "mean_of_square_", "std_"):
        np.testing.assert_array_equal(getattr(back["scaler"], name), getattr(s, name))
    assert "scaler" not in checkpoint.load_models(checkpoint.build_state(crnn, pred, kw, dict(co.PREDICTOR_KWARGS)))


def test_captured_step_with_a_scaler_replays_to_the_eager_result(fes):
    """the device vectors are uploaded at attachment, so the captured step holds no host-to-device copy; the replays
    equal the eager steps bit for bit (helpers and bar of tests/test_graph_step_gpu.py)"""
    from bsed_amd.features import MelFrontEnd
    from test_graph_step_gpu import _compare, _standard_script, _trainer
    fe_s = MelFrontEnd(fes[128].cfg, scaler=_golden_scaler())
    eager, _ = _compare(lambda: _trainer(frontend=fe_s), _standard_script(_waves(4), warmup=2), from_wave=True,
                        what="from_wave with a scaler")
    # and the scaler really is in the step: without it the losses differ
    from bsed_amd.engine import SEDTrainer
    w, y = _waves(1)[0]
    plain = SEDTrainer.loss_value(_trainer(frontend=fes[128]).train_step(w, y, from_wave=True))
    scaled = SEDTrainer.loss_value(_trainer(frontend=fe_s).train_step(w, y, from_wave=True))
    assert plain != scaled
