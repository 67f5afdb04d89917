"""dB-mel with the two rolled ISP views in one pass (csrc/mel.hip ``mel_db_views_kernel``, ``MelFrontEnd.to_db_views`` /
``transform(views=...)``) against the sequence it replaces: ``to_db`` followed by ``ops.roll`` along time / frequency.

No tolerance anywhere: the fused kernel evaluates ``mel_db_kernel``'s dB expression and permutes the result, so its three
outputs must be the same bits (``torch.equal``) as ``to_db`` and its ``bsed_roll`` copies, and as the oracle's per-sample
``torch.roll`` (``oracle.crnn_oracle._roll_each``, the reference's loops of src/main_scmt_ada_weak.py:234-248) of the
base tensor.  The rolls act on the padded / truncated tensor: the 0 dB pad rows travel round with the clip.
"""
import numpy as np
import pytest
import torch

from oracle import crnn_oracle as co
from oracle import mel_oracle as mo

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fe():
    from bsed_amd.features import MelConfig, MelFrontEnd
    return MelFrontEnd(MelConfig(sr=22050))


def _linear_mel(seed, B, T, M=128):
    """seeded linear-mel amplitudes with a wide dynamic range (some below the -80 dB clamp floor, some exact zeros)"""
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(B, T, M, generator=g) * torch.exp(8.0 * torch.rand(B, T, M, generator=g) - 8.0)
    x[:, ::7, 3::11] = 0.0
    x = x * (0.1 + torch.arange(B, dtype=torch.float32)[:, None, None])
    return x.cuda(), x.amax(dim=(1, 2)).cuda()


def _shift_sets(B, T_out):
    """per-sample (frames, bins): zeros, negatives, more than the axis, and the reference's extremes (+-256, +-4)"""
    frames = [0, -8, 12, 256, -256, T_out, T_out + 5, -3 * T_out - 1, 1, -1]
    bins = [0, 3, -2, 4, -4, 128, 131, -257, 1, 127]
    return ([frames[(k + o) % len(frames)] for k in range(B)] for o in (0, 3)), \
           ([bins[(k + o) % len(bins)] for k in range(B)] for o in (0, 5))


def _check(fe, mel, cmax, frames, bins, T_out):
    from bsed_amd import ops
    B, T, M = mel.shape
    base = fe.to_db(mel, cmax, T_out)
    sh = torch.tensor(frames, dtype=torch.int32, device="cuda")
    sw = torch.tensor(bins, dtype=torch.int32, device="cuda")
    x, xt, xf = fe.to_db_views(mel, cmax, frames, bins, T_out)
    assert x.shape == xt.shape == xf.shape == (B, 1, T_out, M)
    assert torch.equal(x, base)
    assert torch.equal(xt, ops.roll(base, B, T_out, M, sh=sh)), (frames, T, T_out)
    assert torch.equal(xf, ops.roll(base, B, T_out, M, sw=sw)), (bins, T, T_out)
    # the oracle's per-sample torch.roll: sample k is (1, T_out, M) -> time is dim 1, frequency dim 2
    cpu = base.cpu()
    assert torch.equal(xt.cpu(), co._roll_each(cpu, frames, 1))
    assert torch.equal(xf.cpu(), co._roll_each(cpu, bins, 2))
    # int32 device tensors are taken as they are
    again = fe.to_db_views(mel, cmax, sh, sw, T_out)
    assert all(torch.equal(a, b) for a, b in zip(again, (x, xt, xf)))


@pytest.mark.parametrize("B,T,T_out", [
    (5, 300, 345),     # T < T_out: 45 pad rows of 0 dB roll round with the clip
    (5, 345, 300),     # T > T_out: truncated, the roll wraps at T_out
    (4, 865, 865),     # T = T_out, the bench clip
    (1, 130, 130),     # a single clip
    (3, 29, 37),       # ragged: T_out = 37 is neither a multiple of the rows per workgroup nor even
    (3, 50, 37),
    (10, 64, 64),      # every entry of the shift tables at once
])
def test_views_equal_to_db_then_roll_bitwise(fe, B, T, T_out):
    mel, cmax = _linear_mel(100 + B + T, B, T)
    fsets, bsets = _shift_sets(B, T_out)
    for frames, bins in zip(fsets, bsets):
        _check(fe, mel, cmax, frames, bins, T_out)


def test_views_without_max_frames_and_all_zero_shifts(fe):
    mel, cmax = _linear_mel(7, 2, 33)
    x, xt, xf = fe.to_db_views(mel, cmax, [0, 0], [0, 0])
    base = fe.to_db(mel, cmax)
    assert x.shape == (2, 1, 33, 128)
    assert torch.equal(x, base) and torch.equal(xt, base) and torch.equal(xf, base)


def test_views_reject_what_the_kernel_is_not_built_for(fe):
    from bsed_amd import _lib as L
    mel, cmax = _linear_mel(8, 2, 16)
    with pytest.raises(L.BsedError):
        fe.to_db_views(mel, cmax, [0], [0, 0])                       # one shift per clip
    with pytest.raises(L.BsedError):
        fe.to_db_views(mel[:, :, :64].contiguous(), cmax, [0, 0], [0, 0])   # rows of 128 bands only


@pytest.mark.parametrize("max_frames", [None, 120])
def test_transform_views_equal_rolls_of_transform(fe, max_frames):
    """waveform -> (clean, noisy) triples == rolls of transform(wav, noisy=True) with the same seed; views=None is
    the transform as it was (same launches)"""
    from bsed_amd import ops
    wav = torch.from_numpy(np.stack([mo.synth_clip(i, sr=22050, seconds=1.0)[0] for i in range(3)])).cuda()
    frames, bins = [-256, 8, 4 * 64], [4, -4, 1]
    clean, noisy = fe.transform(wav, max_frames=max_frames, noisy=True, seed=11)
    vc, vn = fe.transform(wav, max_frames=max_frames, noisy=True, seed=11, views=(frames, bins))
    B, _, T_out, M = clean.shape
    assert T_out == (fe.cfg.max_frames if max_frames is None else max_frames)
    sh = torch.tensor(frames, dtype=torch.int32, device="cuda")
    sw = torch.tensor(bins, dtype=torch.int32, device="cuda")
    for base, (x, xt, xf) in ((clean, vc), (noisy, vn)):
        assert torch.equal(x, base)
        assert torch.equal(xt, ops.roll(base, B, T_out, M, sh=sh))
        assert torch.equal(xf, ops.roll(base, B, T_out, M, sw=sw))
    assert not torch.equal(clean, noisy)
    only = fe.transform(wav, max_frames=max_frames, views=(frames, bins))
    assert len(only) == 3 and all(torch.equal(a, b) for a, b in zip(only, vc))
