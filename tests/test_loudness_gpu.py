"""Integrated loudness on the device (csrc/loudness.hip, ``ops.loudness``, ``features.loudness``) against the sequential
float64 restatement of tests/loudness_reference.py.

One flat buffer per rate (four signals of 1 004 099 samples), 220 segments at odd offsets that overlap one another, in one
launch: lengths 1, 7, half - 1, half, half + sr / 10 - 1, half + sr / 10 (the tiling and the block count stepping 2 -> 3),
10 s, 10 s + 1, the primes 100 003 and 1 000 003 (the kernel's tile is 8192 samples and a workgroup owns 2 .. 32 hops, so
these span many tiles and chunks; 11 025 and 22 050 Hz have uneven hops).  Every case first passes the reference's
margin assertion: no block within 1e-3 LU of a gate, so counts are decided and the value is fixed to round-off.  The bar
is include/bsed.h's: 1e-6 LU, derived there from float64 round-off through the double pole, not from these results."""
import ctypes
import math

import numpy as np
import pytest
import torch

import loudness_reference as lr
from bsed_amd import _lib as L

pytestmark = pytest.mark.gpu

RATES = [11025, 22050, 32000, 44100]
_cache = {}


def _case(sr):
    """(host buffer, device buffer, first sample of each signal, segments, per-segment reference (loud, counts)), built once per
    rate and never modified"""
    if sr not in _cache:
        x, base = lr.gpu_buffer(sr)
        segs = lr.gpu_segments(sr, base)
        ref = []
        for name, off, length in segs:
            loud, counts, margin = lr.loudness_ref(x, off, length, sr)
            lr.assert_decidable(margin, f"{sr} Hz {name} off={off} len={length}")
            ref.append((loud, counts))
        _cache[sr] = (x, torch.from_numpy(x).cuda(), base, segs, ref)
    return _cache[sr]


def _dev_i64(values):
    return torch.tensor(list(values), dtype=torch.int64).cuda()


def _launch(xd, offs, lens, sr, max_len, guard=8):
    """bsed_loudness with caller-made buffers and sentinels behind loud, behind counts and on both sides of the workspace
    -> (loud (S,) float64, counts (S, 3) int32), both on the host, after checking the sentinels"""
    S = len(offs)
    need = L.lib().bsed_loudness_ws_bytes(S, max_len, sr)
    assert need > 0 and need % 8 == 0
    loud = torch.full((S + guard,), 12345.5, dtype=torch.float64, device="cuda")
    counts = torch.full((3 * S + guard,), -77, dtype=torch.int32, device="cuda")
    ws = torch.full((need // 8 + 2 * guard,), -4321.25, dtype=torch.float64, device="cuda")
    seg_off, seg_len = _dev_i64(offs), _dev_i64(lens)            # named: both stay allocated until the results are read
    L.call("bsed_loudness", L.ptr(xd), xd.numel(), L.ptr(seg_off, torch.int64), L.ptr(seg_len, torch.int64), S,
           max_len, sr, ctypes.c_void_p(ws.data_ptr() + 8 * guard), need, L.ptr(loud, torch.float64), L.ptr(counts, torch.int32),
           L.stream())
    assert (loud[S:] == 12345.5).all() and (counts[3 * S:] == -77).all()
    assert (ws[:guard] == -4321.25).all() and (ws[guard + need // 8:] == -4321.25).all()
    return loud[:S].cpu().numpy(), counts[:3 * S].cpu().numpy().reshape(S, 3)


def _check(got, ref, what):
    loud, counts = got
    worst = 0.0
    for k, (want, want_counts) in enumerate(ref):
        assert counts[k].tolist() == want_counts, (what, k, counts[k].tolist(), want_counts)
        if math.isinf(want):
            assert loud[k] == want, (what, k, loud[k])
        else:
            worst = max(worst, abs(loud[k] - want))
            assert abs(loud[k] - want) <= lr.BAR, (what, k, loud[k], want)
    return worst


@pytest.mark.parametrize("sr", RATES)
def test_220_overlapping_segments_in_one_launch(sr):
    x, xd, base, segs, ref = _case(sr)
    offs, lens = [s[1] for s in segs], [s[2] for s in segs]
    assert len(segs) == 220 and all(o % 2 == 1 for o in offs) and max(lens) == lr.LONGEST
    assert sum(math.isinf(r[0]) for r in ref) >= 55 and len({tuple(r[1]) for r in ref}) >= 12
    got = _launch(xd, offs, lens, sr, lr.LONGEST)
    worst = _check(got, ref, f"{sr} Hz")
    print(f"{sr} Hz, S = 220: worst |loud - ref| = {worst:.3e} LU")
    again = _launch(xd, offs, lens, sr, lr.LONGEST)
    assert got[0].tobytes() == again[0].tobytes() and np.array_equal(got[1], again[1])          # two launches: the same bits
    assert np.array_equal(xd.cpu().numpy(), x)                                                  # x is only read
    # the wrapper: the same values, with and without counts
    from bsed_amd import ops
    loud, counts = ops.loudness(xd, _dev_i64(offs), _dev_i64(lens), sr, lr.LONGEST, counts=True)
    assert loud.dtype == torch.float64 and counts.dtype == torch.int32 and counts.shape == (220, 3)
    assert loud.cpu().numpy().tobytes() == got[0].tobytes() and np.array_equal(counts.cpu().numpy(), got[1])
    assert ops.loudness(xd, _dev_i64(offs), _dev_i64(lens), sr, lr.LONGEST).cpu().numpy().tobytes() == got[0].tobytes()


@pytest.mark.parametrize("sr", RATES)
def test_one_segment_per_launch_is_split_over_many_workgroups(sr):
    """S = 1: a workgroup owns two hops, so 10 s are 50 chunks, each warmed up from zero state"""
    x, xd, base, segs, ref = _case(sr)
    worst = 0.0
    for name, length in (("noise_on_dc", 10 * sr + 1), ("noise_on_dc", lr.LONGEST), ("noise", 10 * sr), ("noise", 7),
                         ("sine", (sr + 1) // 2 - 1), ("silence", lr.PRIME)):
        k = next(i for i, s in enumerate(segs) if s[0] == name and s[2] == length)
        got = _launch(xd, [segs[k][1]], [length], sr, length)
        worst = max(worst, _check(got, [ref[k]], f"{sr} Hz {name} {length}"))
    print(f"{sr} Hz, S = 1: worst |loud - ref| = {worst:.3e} LU")


@pytest.mark.parametrize("sr", [11025, 32000])
def test_max_len_cuts_a_segment_and_indices_outside_the_buffer_read_zero(sr):
    x, xd, base, segs, _ = _case(sr)
    n, half = len(x), (sr + 1) // 2
    b = base["noise_on_dc"]
    max_len = 7 * sr + 13
    cases = [(b + 3, 10 * sr), (b + 5, max_len), (b + 7, max_len - 1), (b + 9, half - 1),      # cut; at the bound; below it
             (n - 5001, 3 * sr), (n + 11, sr), (-777, 2 * sr), (-5 * sr, sr), (b + 1, 0), (b + 1, -3)]
    ref = []
    for off, length in cases:
        loud, counts, margin = lr.loudness_ref(x, off, length, sr, max_len=max_len)
        lr.assert_decidable(margin, f"{sr} Hz off={off} len={length}")
        ref.append((loud, counts))
    assert ref[5][0] == -math.inf and ref[7][0] == -math.inf and ref[8] == (-math.inf, [0, 0, 0]) and ref[9] == ref[8]
    assert math.isfinite(ref[4][0]) and math.isfinite(ref[6][0])
    got = _launch(xd, [c[0] for c in cases], [c[1] for c in cases], sr, max_len)
    _check(got, ref, f"{sr} Hz max_len")
    # a bound below half a second: every segment is its first 100 samples, tiled
    tiny = [(b + 3, 10 * sr), (b + 3, 100), (b + 3, 99)]
    ref = []
    for off, length in tiny:
        loud, counts, margin = lr.loudness_ref(x, off, length, sr, max_len=100)
        lr.assert_decidable(margin, f"{sr} Hz off={off} len={length} cut to 100")
        ref.append((loud, counts))
    got = _launch(xd, [c[0] for c in tiny], [c[1] for c in tiny], sr, 100)
    _check(got, ref, f"{sr} Hz max_len = 100")
    assert got[0][0] == got[0][1]


def test_features_loudness_of_batches_int16_and_single_waveforms():
    from bsed_amd import features
    sr, n = 32000, 2 * 32000 + 17
    rng = np.random.default_rng(9)
    waves = np.stack([0.1 * rng.standard_normal(n), 0.01 * rng.standard_normal(n) + 0.2, np.zeros(n),
                      0.3 * np.sin(2 * np.pi * 440.0 * np.arange(n) / sr)]).astype(np.float32)
    ref = []
    for row in waves:
        loud, _, margin = lr.loudness_of(row, sr)
        lr.assert_decidable(margin)
        ref.append(loud)
    got = features.loudness(waves, sr)
    assert got.is_cuda and got.dtype == torch.float64 and got.shape == (4,)
    got = got.cpu().numpy()
    assert got[2] == -math.inf and np.abs(np.delete(got, 2) - np.delete(ref, 2)).max() <= lr.BAR
    assert features.loudness(torch.from_numpy(waves).cuda(), sr).cpu().numpy().tobytes() == got.tobytes()
    one = features.loudness(waves[0], sr)
    assert one.shape == (1,) and abs(float(one[0]) - ref[0]) <= lr.BAR
    # int16: converted as load_audio converts it, (float)s * (1 / 32768) in fp32
    pcm = np.round(waves * 20000.0).astype(np.int16)
    want = [lr.loudness_of(row.astype(np.float32) * np.float32(1.0 / 32768.0), sr)[0] for row in pcm]
    got16 = features.loudness(pcm, sr).cpu().numpy()
    assert got16[2] == -math.inf and np.abs(np.delete(got16, 2) - np.delete(want, 2)).max() <= lr.BAR
    for bad, word in ((np.zeros((2, 3, 4), np.float32), "shape"), (np.zeros(10), "float64"), ([0.0], "numpy"),
                      (np.zeros((0, 5), np.float32), "shape")):
        with pytest.raises(L.BsedError, match=word):
            features.loudness(bad, sr)


def test_normalize_loudness_reaches_the_target_and_leaves_silence_alone():
    """the scaled rows measure the target to within the float32 rounding of one gain and of the products: 2^-24 relative in
    the gain is 5e-7 dB, and the products' roundings are independent per sample; 1e-5 LU leaves a decade of room"""
    from bsed_amd import features
    sr, n = 22050, 3 * 22050
    rng = np.random.default_rng(4)
    waves = np.stack([0.05 * rng.standard_normal(n), np.zeros(n), 0.5 * rng.standard_normal(n)]).astype(np.float32)
    scaled, lufs = features.normalize_loudness(waves, sr, -23.0)
    assert scaled.shape == (3, n) and scaled.dtype == torch.float32 and lufs.shape == (3,) and lufs.dtype == torch.float64
    before = features.loudness(waves, sr)
    assert torch.equal(lufs, before) and lufs[1] == -math.inf
    out = scaled.cpu().numpy()
    assert not out[1].any()
    for k in (0, 2):
        loud, _, margin = lr.loudness_of(out[k], sr)
        lr.assert_decidable(margin)
        assert abs(loud - (-23.0)) <= 1e-5, (k, loud)
    single, l1 = features.normalize_loudness(waves[2], sr, -30.0)
    assert single.shape == (n,) and abs(lr.loudness_of(single.cpu().numpy(), sr)[0] + 30.0) <= 1e-5 and l1.shape == (1,)
