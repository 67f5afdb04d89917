"""Resampling on the GPU: ``bsed_resample_poly`` through ``features.Resampler`` against the float64 restatement of
tests/resample_reference.py, element by element, within the fp32 accumulation bound

    |y[m] - ref[m]| <= (K[m] + 2) * 2^-24 * S[m],      S = sum |x[j]| |tap|,  K = the number of terms

which holds for a sum of K fp32 products in ANY order (the reference sees the same fp32 taps and the same fp32 mono
samples as the kernel).  Worst ratio measured on an MI355X over every case of
``test_accuracy_against_the_float64_restatement``: see DESIGN.md, "Resampling".  The filter is the project's own: nothing
here compares against librosa or soxr."""
import wave

import numpy as np
import pytest
import torch

from resample_reference import RATE_PAIRS, U24, mono_f32, n_out, resample_ref, taps32

pytestmark = pytest.mark.gpu


def _rs(sr_in, sr_out, **kw):
    from bsed_amd.features import resampler
    return resampler(sr_in, sr_out, **kw)


def _against_ref(y, x, rs, idx=None, what=""):
    """assert the bound at ``idx`` (default: every output) -> worst |y - ref| / bound"""
    y = y.cpu().numpy() if isinstance(y, torch.Tensor) else y
    assert y.dtype == np.float32 and y.shape == (rs.n_out(len(x)),), (what, y.shape)
    ref, S, K = resample_ref(mono_f32(x), taps32(rs.taps), rs.up, rs.down, rs.half_len, idx=idx)
    got = y.astype(np.float64) if idx is None else y[idx].astype(np.float64)
    assert np.all(np.isfinite(got)), what
    err, bound = np.abs(got - ref), (K + 2) * U24 * S
    ratio = float((err[bound > 0] / bound[bound > 0]).max()) if np.any(bound > 0) else 0.0
    print(f"{what}: worst |y - ref| / bound = {ratio:.4f} (max |err| {err.max():.3e}, K up to {K.max()})")
    assert np.all(err <= bound), (what, ratio, int(np.argmax(err - bound)))
    return ratio


def _families(sr_in, n, seed):
    rng = np.random.default_rng(seed)
    t = np.arange(n) / sr_in
    f1 = sr_in / 2.0
    sweep = np.sin(2 * np.pi * (50.0 * t + (f1 - 50.0) / (2 * t[-1]) * t * t))      # 50 Hz -> sr_in / 2, linear
    imp = np.zeros(n, np.float32)
    imp[0], imp[-1] = 1.0, -0.75
    full = rng.integers(-32768, 32768, n).astype(np.int16)
    full[::7], full[3::11] = -32768, 32767
    return [("noise", rng.standard_normal(n).astype(np.float32)), ("sweep", sweep.astype(np.float32)), ("impulses", imp),
            ("constant", np.full(n, 0.8, np.float32)), ("int16_full_scale", full)]


# ---------------------------------------------------------------------------------------------------------------------
# accuracy
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sr_in,sr_out", RATE_PAIRS)
def test_accuracy_against_the_float64_restatement(sr_in, sr_out):
    rs = _rs(sr_in, sr_out)
    worst = 0.0
    for name, x in _families(sr_in, 30011, seed=sr_in + sr_out):
        worst = max(worst, _against_ref(rs(x), x, rs, what=f"{sr_in}->{sr_out} {name}"))
    print(f"{sr_in}->{sr_out}: worst ratio over the input families {worst:.4f}")


def test_accuracy_of_a_60_db_filter():
    rs = _rs(44100, 32000, attenuation_db=60.0)
    x = np.random.default_rng(1).standard_normal(20000).astype(np.float32)
    assert rs.taps_per_phase < _rs(44100, 32000).taps_per_phase
    _against_ref(rs(x), x, rs, what="44100->32000 at 60 dB")


# ---------------------------------------------------------------------------------------------------------------------
# formats
# ---------------------------------------------------------------------------------------------------------------------
def test_formats_channels_and_containers():
    rs = _rs(44100, 32000)
    rng = np.random.default_rng(2)
    m16 = rng.integers(-32768, 32768, 20001).astype(np.int16)
    y16 = rs(m16)
    assert torch.equal(y16, rs((m16 / 32768.0).astype(np.float32)))                  # int16 mono == float32 x / 32768
    assert torch.equal(y16, rs(m16[:, None]))                                        # (n, 1) == (n,)
    assert torch.equal(y16, rs(torch.from_numpy(m16).cuda()))                        # numpy == GPU tensor
    left = rng.integers(-32767, 32768, 20001).astype(np.int16)
    zero = rs(np.stack([left, -left], axis=1))
    assert torch.count_nonzero(zero) == 0                                            # R = -L: exact zeros
    f = rng.standard_normal(20001).astype(np.float32)
    assert torch.count_nonzero(rs(np.stack([f, -f], axis=1))) == 0
    assert torch.equal(rs(f), rs(torch.from_numpy(f).cuda())) and torch.equal(rs(f), rs(f[:, None]))
    for ch in (2, 3, 6):
        xi = rng.integers(-32768, 32768, (9001, ch)).astype(np.int16)
        _against_ref(rs(xi), xi, rs, what=f"int16 {ch} channels")
        xf = rng.standard_normal((9001, ch)).astype(np.float32)
        _against_ref(rs(xf), xf, rs, what=f"float32 {ch} channels")
        assert torch.equal(rs(xf), rs(torch.from_numpy(xf).cuda()))
    # a view with strides is made contiguous, not misread
    wide = torch.from_numpy(rng.standard_normal((9001, 4)).astype(np.float32)).cuda()
    assert torch.equal(rs(wide[:, :2]), rs(wide[:, :2].contiguous()))


# ---------------------------------------------------------------------------------------------------------------------
# lengths and edges
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sr_in,sr_out", [(48000, 32000), (44100, 32000), (44100, 22050), (22050, 32000)])
def test_lengths_that_fit_no_block_size(sr_in, sr_out):
    rs = _rs(sr_in, sr_out)
    rng = np.random.default_rng(5)
    tile_in = 1024 * rs.down // rs.up                # input frames of one workgroup's 1024 outputs, roughly
    for n in sorted({1, 2, rs.down - 1, rs.down + 1, rs.down, 7919, tile_in - 1, tile_in, tile_in + 1, 16 * rs.down,
                     16 * rs.down + 1, 3 * tile_in + 5} - {0}):
        x = rng.standard_normal(n).astype(np.float32)
        _against_ref(rs(x), x, rs, what=f"{sr_in}->{sr_out} n_in={n}")


@pytest.mark.parametrize("fmt", ["int16", "float32"])
def test_nothing_is_written_behind_the_last_output(fmt):
    from bsed_amd import _lib as L
    rs = _rs(44100, 32000)
    rng = np.random.default_rng(6)
    for n in (1, 440, 7919, 30011):
        x = rng.integers(-32768, 32768, (n, 2)).astype(np.int16) if fmt == "int16" else rng.standard_normal((n, 2)).astype(np.float32)
        xd = torch.from_numpy(x).cuda()
        no = rs.n_out(n)
        buf = torch.full((no + 4096,), -12345.0, device="cuda")
        table = torch.from_numpy(rs.table).cuda()
        L.call("bsed_resample_poly", L.ptr(xd, xd.dtype), L.CONSTANTS["BSED_PCM_S16" if fmt == "int16" else "BSED_PCM_F32"],
               n, 2, L.ptr(table), rs.up, rs.down, rs.half_len, L.ptr(buf), no, L.stream())
        assert torch.all(buf[no:] == -12345.0)
        assert torch.equal(buf[:no], rs(x))


# ---------------------------------------------------------------------------------------------------------------------
# long index: m * down passes 2^32
# ---------------------------------------------------------------------------------------------------------------------
def test_fourteen_million_frames_index_past_32_bits():
    rs = _rs(44100, 32000)
    n = 14_000_000
    rng = np.random.default_rng(14)
    x = rng.integers(-32768, 32768, n).astype(np.int16)
    y = rs(x)
    no = rs.n_out(n)
    assert (no - 1) * rs.down > 2 ** 32
    idx = np.unique(np.concatenate([rng.integers(0, no, 4096), np.arange(no - 512, no)]))
    assert np.count_nonzero(idx * rs.down > 2 ** 32) >= 512
    _against_ref(y, x, rs, idx=idx, what="14e6 frames 44100->32000")          # every sampled index is compared
    del y


# ---------------------------------------------------------------------------------------------------------------------
# filter quality through the kernel
# ---------------------------------------------------------------------------------------------------------------------
def test_a_1_khz_tone_keeps_its_amplitude_and_a_20_khz_tone_is_rejected():
    rs = _rs(48000, 32000)
    n = 48000
    t = np.arange(n) / 48000.0
    edge = 2 * rs.taps_per_phase                       # outputs whose taps reach past either end of the signal
    ripple = 10 ** (1e-3 / 20) - 1                     # the pass-band bound of tests/test_resample_cpu.py, as a ratio
    x = np.sin(2 * np.pi * 1000.0 * t).astype(np.float32)
    y = rs(x).cpu().numpy()
    ref, S, K = resample_ref(mono_f32(x), taps32(rs.taps), rs.up, rs.down, rs.half_len)
    ideal = np.sin(2 * np.pi * 1000.0 * np.arange(len(y)) / 32000.0)
    inner = slice(edge, len(y) - edge)
    assert np.abs(ref[inner] - ideal[inner]).max() <= ripple + 2 * U24        # + the fp32 rounding of the input tone
    assert np.all(np.abs(y[inner] - ideal[inner]) <= ripple + 2 * U24 + ((K + 2) * U24 * S)[inner])
    _against_ref(y, x, rs, what="1 kHz tone")
    # 20 kHz at 48 k lies above the new Nyquist and would alias to 12 kHz
    x = np.sin(2 * np.pi * 20000.0 * t).astype(np.float32)
    y = rs(x).cpu().numpy()
    ref, S, K = resample_ref(mono_f32(x), taps32(rs.taps), rs.up, rs.down, rs.half_len)
    level = 20 * np.log10(np.abs(ref[inner]).max())
    print(f"20 kHz tone through 48000->32000: {level:.1f} dB relative to the input")
    assert level < -99.0
    _against_ref(y, x, rs, what="20 kHz tone")


# ---------------------------------------------------------------------------------------------------------------------
# determinism, identity
# ---------------------------------------------------------------------------------------------------------------------
def test_two_runs_and_another_stream_give_the_same_bits():
    rng = np.random.default_rng(8)
    for pair in ((48000, 32000), (44100, 32000)):
        rs = _rs(*pair)
        x = torch.from_numpy(rng.integers(-32768, 32768, (200003, 2)).astype(np.int16)).cuda()
        a, b = rs(x), rs(x)
        assert torch.equal(a, b)
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            c = rs(x)
        s.synchronize()
        assert torch.equal(a, c)


def test_equal_rates_pass_mono_float32_through_and_convert_everything_else_exactly():
    from bsed_amd import ops
    rs = _rs(32000, 32000)
    rng = np.random.default_rng(9)
    f = torch.from_numpy(rng.standard_normal(5000).astype(np.float32)).cuda()
    assert rs(f) is f
    assert rs.n_out(5000) == 5000
    st = rng.integers(-32768, 32768, (5003, 2)).astype(np.int16)
    want = st.astype(np.int32).sum(axis=1).astype(np.float32) * np.float32(1.0 / 65536.0)   # exact: a power of two
    assert np.array_equal(rs(st).cpu().numpy(), want)
    assert np.array_equal(rs(st[:, 0].copy()).cpu().numpy(), st[:, 0].astype(np.float32) / np.float32(32768.0))
    f3 = rng.standard_normal((5003, 3)).astype(np.float32)
    assert np.array_equal(rs(f3).cpu().numpy(), mono_f32(f3))
    # the launch announces its work to the kernel timer as the other wrappers do
    seen = []

    class Timer:
        def launch(self, key, flops, fn, nbytes):
            seen.append((key, flops, nbytes))
            fn()

    ops.set_timer(Timer())
    try:
        _rs(48000, 32000)(st)
    finally:
        ops.set_timer(None)
    (key, flops, nbytes), = seen
    assert key[0].startswith("resample_poly_kernel") and flops == 2.0 * 3336 * 215 and nbytes == 5003 * 4 + 3336 * 4 + 2 * 215 * 4


# ---------------------------------------------------------------------------------------------------------------------
# load_audio, detect_recording
# ---------------------------------------------------------------------------------------------------------------------
def _stereo48(seconds=24.0):
    from test_detect_gpu import recording
    w = recording(seconds, sr=48000)
    left = np.clip(np.round(w * 20000.0), -32768, 32767).astype(np.int16)
    right = np.clip(np.round(np.roll(w, 7) * 12000.0), -32768, 32767).astype(np.int16)
    return np.stack([left, right], axis=1)


def test_load_audio_is_read_wav_plus_one_resampler_launch(tmp_path):
    from bsed_amd.features import load_audio
    x = _stereo48(3.0)
    path = tmp_path / "field.wav"
    with wave.open(str(path), "wb") as f:
        f.setnchannels(2); f.setsampwidth(2); f.setframerate(48000)
        f.writeframes(x.astype("<i2").tobytes())
    y, sr = load_audio(path)
    assert sr == 32000 and y.is_cuda and y.dtype == torch.float32 and y.shape == (n_out(len(x), 2, 3),)
    assert torch.equal(y, _rs(48000, 32000)(x))
    y22, sr22 = load_audio(str(path), sr=22050, attenuation_db=60.0)
    assert sr22 == 22050 and torch.equal(y22, _rs(48000, 22050, attenuation_db=60.0)(x))


def test_detect_recording_resamples_first_and_is_unchanged_without_sr():
    from bsed_amd.evaluation import detect_recording
    from bsed_amd.features import MelFrontEnd
    from bsed_amd.labels import BIRD_LIST, ManyHotEncoder
    from test_detect_gpu import _models, recording
    fe, enc = MelFrontEnd(), ManyHotEncoder(BIRD_LIST, n_frames=313)
    _, _, crnn, pred = _models()
    kw = dict(predictor=pred, mel=fe, batch_windows=4, return_probabilities=True)
    w48 = _stereo48()
    ev1, ev2 = [], []
    df1, st1, wp1 = detect_recording(crnn, w48, enc.decode_strong, sr=48000, stage_events=ev1, **kw)
    wave32 = _rs(48000, fe.cfg.sr)(w48)
    df2, st2, wp2 = detect_recording(crnn, wave32, enc.decode_strong, stage_events=ev2, **kw)
    assert wp1.shape[0] >= 3 and torch.equal(wp1, wp2) and torch.equal(st1, st2)
    assert df1.equals(df2) and (len(df1) == 0 or df1["offset"].max() <= wave32.numel() / fe.cfg.sr)
    assert [n for n, _, _ in ev1].count("resample") == 1 and ev1[0][0] == "resample"
    assert "resample" not in [n for n, _, _ in ev2]
    # the GPU tensor form of the same recording, and a quality setting that reaches the filter
    df3, st3, _ = detect_recording(crnn, torch.from_numpy(w48).cuda(), enc.decode_strong, sr=48000, **kw)
    assert torch.equal(st3, st1) and df3.equals(df1)
    _, st60, _ = detect_recording(crnn, w48, enc.decode_strong, sr=48000, resample_quality={"attenuation_db": 60.0}, **kw)
    _, st60b, _ = detect_recording(crnn, _rs(48000, fe.cfg.sr, attenuation_db=60.0)(w48), enc.decode_strong, **kw)
    assert torch.equal(st60, st60b)
    # float32 mono at the model's rate: sr=None and sr=cfg.sr are today's call, bit for bit, without a resample stage
    w32 = recording(24.0)
    ev4, ev5 = [], []
    df4, st4, wp4 = detect_recording(crnn, w32, enc.decode_strong, stage_events=ev4, **kw)
    df5, st5, wp5 = detect_recording(crnn, w32, enc.decode_strong, sr=fe.cfg.sr, stage_events=ev5, **kw)
    assert torch.equal(st4, st5) and torch.equal(wp4, wp5) and df4.equals(df5)
    assert "resample" not in [n for n, _, _ in ev4] + [n for n, _, _ in ev5]
    assert [n for n, _, _ in ev4] == [n for n, _, _ in ev5]
    assert crnn.training and pred.training
