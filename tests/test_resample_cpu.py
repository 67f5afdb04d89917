"""Resampling, the part that needs no GPU: the filter design against its specification and its measured response, the
float64 restatement (tests/resample_reference.py) against scipy.signal.resample_poly as a second source, ``read_wav``,
and the argument checks of ``bsed_resample_poly`` and ``detect_recording(sr=...)``, which run before any HIP call.
The filter is the project's own; nothing here compares against librosa or soxr."""
import math
import wave

import numpy as np
import pytest

from bsed_amd import _lib as L
from bsed_amd.features import Resampler, resample_filter, resample_table
from resample_reference import RATE_PAIRS, U53, UP_DOWN, n_out, resample_ref, response_db


# ---------------------------------------------------------------------------------------------------------------------
# filter design
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sr_in,sr_out", RATE_PAIRS)
def test_filter_meets_its_specification(sr_in, sr_out):
    taps, up, down, half_len = resample_filter(sr_in, sr_out)
    assert (up, down) == UP_DOWN[(sr_in, sr_out)]
    assert taps.dtype == np.float64 and len(taps) == 2 * half_len + 1 and len(taps) % 2 == 1
    assert np.array_equal(taps, taps[::-1])
    # the length by the formula, spelled out once more
    low = min(sr_in, sr_out)
    N = math.ceil((100.0 - 8.0) / (2.285 * 2 * math.pi * (low / 2 - 0.91 * low / 2) / (sr_in * up)))
    assert half_len == (N + 1) // 2
    stop, ripple = response_db(taps, up, sr_in, sr_out)
    print(f"{sr_in}->{sr_out}: up={up} down={down} half_len={half_len} stop band {stop:.2f} dB, ripple {ripple:.2e} dB")
    assert stop <= -99.5                # measured -99.8 at worst; 0.3 dB for the placement of the FFT grid
    assert ripple <= 1e-3               # measured 1.7e-4
    phase_sums = np.array([taps[r::up].sum() for r in range(up)])
    assert np.abs(phase_sums - 1.0).max() <= 1e-5       # measured 1.35e-6


@pytest.mark.parametrize("sr_in,sr_out", [(48000, 32000), (44100, 32000)])
def test_a_60_db_filter_is_shorter_and_meets_60_db(sr_in, sr_out):
    t100, up, _, h100 = resample_filter(sr_in, sr_out)
    t60, up60, _, h60 = resample_filter(sr_in, sr_out, attenuation_db=60.0)
    assert up60 == up and h60 < h100 and len(t60) == 2 * h60 + 1
    stop, _ = response_db(t60, up, sr_in, sr_out)
    assert stop <= -59.5


def test_filter_refuses_bad_arguments():
    for bad in (0.0, 1.0, -0.5, 1.2):
        with pytest.raises(L.BsedError, match="rolloff"):
            resample_filter(48000, 32000, rolloff=bad)
    for a, b in ((0, 32000), (48000, 0), (-1, 32000), (48000.5, 32000)):
        with pytest.raises(L.BsedError, match="sr_"):
            resample_filter(a, b)
    with pytest.raises(L.BsedError, match="attenuation_db"):
        resample_filter(48000, 32000, attenuation_db=10.0)
    with pytest.raises(L.BsedError, match="rolloff"):
        Resampler(48000, 32000, rolloff=1.5)


@pytest.mark.parametrize("sr_in,sr_out", RATE_PAIRS)
def test_table_holds_the_taps_by_output_residue(sr_in, sr_out):
    taps, up, down, half_len = resample_filter(sr_in, sr_out)
    table = resample_table(taps, up, down, half_len)
    P = (2 * half_len) // up + 1
    assert table.shape == (up, P) and table.dtype == np.float32
    for c in sorted({0, 1 % up, up // 2, up - 1}):
        r = (c * down + half_len) % up
        want = np.zeros(P)
        col = taps[r::up]
        want[:len(col)] = col
        assert np.array_equal(table[c], want.astype(np.float32))
    # every tap sits in the table exactly once
    assert np.count_nonzero(table) == np.count_nonzero(taps.astype(np.float32))
    rs = Resampler(sr_in, sr_out)
    assert rs.taps_per_phase == P and rs.n_out(1000) == n_out(1000, up, down)
    one = Resampler(sr_in, sr_in)
    assert (one.up, one.down, one.half_len) == (1, 1, 0) and one.table.tolist() == [[1.0]]


# ---------------------------------------------------------------------------------------------------------------------
# the restatement against scipy
# ---------------------------------------------------------------------------------------------------------------------
def _inputs(down, n=3000):
    rng = np.random.default_rng(down)
    imp0, imp1 = np.zeros(n), np.zeros(n)
    imp0[0], imp1[-1] = 1.0, 1.0
    out = [("noise", rng.standard_normal(n)), ("impulse_first", imp0), ("impulse_last", imp1), ("constant", np.ones(n))]
    for k in sorted({1, 2, down - 1, down, down + 1}):
        if k >= 1:
            out.append((f"n{k}", rng.standard_normal(k)))
    return out


@pytest.mark.parametrize("sr_in,sr_out", RATE_PAIRS)
def test_restatement_agrees_with_scipy_resample_poly(sr_in, sr_out):
    from scipy.signal import resample_poly
    taps, up, down, half_len = resample_filter(sr_in, sr_out)
    worst = 0.0
    for name, x in _inputs(down):
        y, S, K = resample_ref(x, taps, up, down, half_len)
        z = resample_poly(x, up, down, window=taps / up, padtype="constant")
        assert z.dtype == np.float64 and len(z) == len(y) == n_out(len(x), up, down), name
        bound = 4 * K * U53 * S
        err = np.abs(y - z)
        assert np.all(err <= bound), (name, float(err.max()), int(np.argmax(err - bound)))
        worst = max(worst, float((err[bound > 0] / bound[bound > 0]).max()))
        assert K.max() <= (2 * half_len) // up + 1 and (len(x) < 3000 or K.max() == (2 * half_len) // up + 1)
    print(f"{sr_in}->{sr_out}: worst |restatement - scipy| / bound = {worst:.3f}")


def test_restatement_on_a_subset_of_outputs_and_by_hand():
    taps, up, down, half_len = resample_filter(44100, 32000)
    x = np.random.default_rng(3).standard_normal(5000)
    y, S, K = resample_ref(x, taps, up, down, half_len)
    idx = np.array([0, 1, 17, 3000, len(y) - 1])
    ys, Ss, Ks = resample_ref(x, taps, up, down, half_len, idx=idx)
    assert np.array_equal(ys, y[idx]) and np.array_equal(Ss, S[idx]) and np.array_equal(Ks, K[idx])
    # one output, term by term from the definition
    m = 1234
    tot, cnt = 0.0, 0
    for j in range(len(x)):
        t = m * down - j * up + half_len
        if 0 <= t <= 2 * half_len:
            tot += x[j] * taps[t]
            cnt += 1
    assert cnt == K[m] and abs(tot - y[m]) <= 4 * cnt * U53 * S[m]
    # up = down = 1 with the single tap: the identity
    yi, Si, Ki = resample_ref(x, np.ones(1), 1, 1, 0)
    assert np.array_equal(yi, x) and np.array_equal(Si, np.abs(x)) and np.all(Ki == 1)


# ---------------------------------------------------------------------------------------------------------------------
# read_wav
# ---------------------------------------------------------------------------------------------------------------------
def _write_wav(path, data, sr, width=2):
    with wave.open(str(path), "wb") as f:
        f.setnchannels(1 if data.ndim == 1 else data.shape[1])
        f.setsampwidth(width)
        f.setframerate(sr)
        f.writeframes(data.tobytes() if width == 2 else bytes(data.size * width))


def test_read_wav_round_trips_pcm16_and_refuses_other_widths(tmp_path):
    from bsed_amd.data import read_wav
    rng = np.random.default_rng(0)
    mono = rng.integers(-32768, 32768, 4001).astype("<i2")
    stereo = rng.integers(-32768, 32768, (3000, 2)).astype("<i2")
    _write_wav(tmp_path / "m.wav", mono, 44100)
    _write_wav(tmp_path / "s.wav", stereo, 48000)
    x, sr = read_wav(tmp_path / "m.wav")
    assert sr == 44100 and x.dtype == np.int16 and x.shape == (4001, 1) and np.array_equal(x[:, 0], mono)
    x, sr = read_wav(str(tmp_path / "s.wav"))
    assert sr == 48000 and x.dtype == np.int16 and x.shape == (3000, 2) and np.array_equal(x, stereo) and x.flags.writeable
    for width in (1, 3):
        _write_wav(tmp_path / f"w{width}.wav", mono, 44100, width=width)
        with pytest.raises(L.BsedError, match=f"{8 * width}-bit"):
            read_wav(tmp_path / f"w{width}.wav")


# ---------------------------------------------------------------------------------------------------------------------
# C ABI: declared in the header, every argument check before the first HIP call
# ---------------------------------------------------------------------------------------------------------------------
def test_resample_entry_point_is_declared_and_refuses_bad_arguments_before_any_hip_call():
    lib = L.lib()
    assert lib.bsed_abi_version() >= 5
    assert "bsed_resample_poly" in L.header_symbols()
    assert (L.CONSTANTS["BSED_PCM_F32"], L.CONSTANTS["BSED_PCM_S16"]) == (0, 1)
    assert len(L.FUNCTIONS["bsed_resample_poly"][1]) == 11
    F32, S16 = L.CONSTANTS["BSED_PCM_F32"], L.CONSTANTS["BSED_PCM_S16"]
    d, tab, out = 0x100000, 0x10000, 0x4000000        # non-null, aligned, far apart, never dereferenced on the host

    def refused(rc, word):
        msg = lib.bsed_last_error().decode()
        assert rc == -1 and word in msg, (rc, msg)

    ok = dict(n_in=48000, ch=2, up=2, down=3, half=322, n_out=32000)
    call = lambda **k: (lambda a: lib.bsed_resample_poly(a["inp"], a["fmt"], a["n_in"], a["ch"], a["tab"], a["up"], a["down"],
                                                         a["half"], a["out"], a["n_out"], None))(
        {**dict(inp=d, fmt=S16, tab=tab, out=out), **ok, **k})
    refused(call(inp=None), "null")
    refused(call(tab=None), "null")
    refused(call(out=None), "null")
    refused(call(n_in=0, n_out=0), "n_in")
    refused(call(ch=0), "channels")
    refused(call(ch=65), "channels")
    refused(call(fmt=2), "format")
    refused(call(fmt=-1), "format")
    refused(call(up=0), "up and down")
    refused(call(down=0), "up and down")
    refused(call(up=4, down=6, n_out=32000), "coprime")
    refused(call(n_out=31999), "n_out")
    refused(call(n_out=32001), "n_out")
    refused(call(n_in=48001, n_out=32000), "n_out")                   # ceil(48001 * 2 / 3) = 32001
    refused(call(out=d + 48000 * 2 * 2 - 4), "overlap")               # the output starts inside the int16 input
    refused(call(fmt=F32, out=d + 48000 * 2 * 4 - 4), "overlap")
    refused(call(inp=out + 4 * 32000 - 2), "overlap")                 # the input starts inside the output
    refused(call(inp=out, out=out), "overlap")
    # a table that the layout cannot stage: 2 * 30000 + 1 taps in one phase; 44.1 k -> 8 k at 100 dB (785 taps per phase)
    refused(call(up=1, down=1, half=30000, n_out=48000), "too large")
    refused(call(n_in=44100, up=80, down=441, half=31400, n_out=8000), "too large")


def test_python_resampler_refuses_bad_inputs_before_any_gpu_call():
    import torch
    rs = Resampler(48000, 32000)
    for bad, word in ((np.zeros(100, np.float64), "float64"), (np.zeros(100, np.int32), "int32"),
                      (np.zeros((10, 2, 2), np.float32), "shape"), (np.zeros((100, 65), np.int16), "channels"),
                      (np.zeros(0, np.float32), "frame"), ([0.0, 1.0], "numpy"),
                      (torch.zeros(100, dtype=torch.float64), "float64")):
        with pytest.raises(L.BsedError, match=word):
            rs(bad)


class _Enc:
    from oracle import labels_oracle as _lo
    labels = _lo.BIRD_LIST

    def decode_strong(self, y):
        return self._lo.decode_strong(y)


class _Mel:
    class cfg:
        sr, hop_size, max_len_seconds = 32000, 255, 10.0


def test_detect_recording_refuses_bad_resampling_arguments_before_any_hip_call():
    import torch
    from bsed_amd import evaluation as ev
    stereo = np.zeros((96000, 2), np.int16)

    def run(wave, **kw):
        return ev.detect_recording(torch.nn.Identity(), wave, _Enc().decode_strong, predictor=torch.nn.Identity(), mel=_Mel(),
                                   **kw)

    for sr in (0, -48000, 48000.5, "48000", True):
        with pytest.raises(L.BsedError, match="sr must"):
            run(stereo, sr=sr)
    with pytest.raises(L.BsedError, match="resample_quality needs sr"):
        run(np.zeros(96000, np.float32), resample_quality={"rolloff": 0.9})
    with pytest.raises(L.BsedError, match="resample_quality"):
        run(stereo, sr=48000, resample_quality={"quality": "high"})
    with pytest.raises(L.BsedError, match="resample_quality"):
        run(stereo, sr=48000, resample_quality=0.9)
    with pytest.raises(L.BsedError, match="rolloff"):
        run(stereo, sr=48000, resample_quality={"rolloff": 1.5})
    with pytest.raises(L.BsedError, match="float64"):
        run(np.zeros((96000, 2)), sr=48000)
    with pytest.raises(L.BsedError, match="shape"):
        run(np.zeros((10, 2, 2), np.int16), sr=48000)
    with pytest.raises(L.BsedError, match="channels"):
        run(np.zeros((1000, 65), np.int16), sr=48000)
    with pytest.raises(L.BsedError, match="hop_frames"):            # the existing checks still apply to the resampled length
        run(stereo, sr=48000, hop_frames=400)
    with pytest.raises(L.BsedError, match="mono waveform"):          # without sr, a stereo array is still refused
        run(np.zeros((96000, 2), np.float32))
