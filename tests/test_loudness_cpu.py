"""Integrated loudness, the part that needs no GPU: the C ABI (declared, exported, every refusal before any HIP call),
the host-side coefficients against the float64 restatement, and the LUFS gains of ``plan_soundscapes`` over a bank
described by its tables alone."""
import ctypes
import math

import numpy as np
import pytest

import loudness_reference as lr
from bsed_amd import _lib as L
from bsed_amd import synth
from bsed_amd.labels import BIRD_LIST


def test_entry_points_are_declared_and_exported():
    lib = L.lib()
    assert lib.bsed_abi_version() >= 15
    for name, nargs in (("bsed_kweight_coefs", 2), ("bsed_loudness_ws_bytes", 3), ("bsed_loudness", 12)):
        assert name in L.header_symbols() and hasattr(lib, name)
        assert len(L.FUNCTIONS[name][1]) == nargs
    assert L.FUNCTIONS["bsed_loudness_ws_bytes"][0] is ctypes.c_long


def test_loudness_refuses_bad_arguments_before_any_hip_call():
    lib = L.lib()
    x, off, ln, ws, loud, cnt = 0x100000, 0x200000, 0x300000, 0x400000, 0x500000, 0x600000   # aligned, never dereferenced
    need = lib.bsed_loudness_ws_bytes(4, 320000, 32000)
    assert need == 8 * 4 * 100                                   # 100 whole hops in 10 s

    def refused(rc, word):
        msg = lib.bsed_last_error().decode()
        assert rc == -1 and msg.startswith("bsed_loudness") and word in msg, (rc, msg)

    ok = dict(x=x, x_len=10 ** 6, off=off, ln=ln, S=4, max_len=320000, sr=32000, ws=ws, ws_bytes=need, loud=loud, cnt=cnt)
    call = lambda **k: (lambda a: lib.bsed_loudness(a["x"], a["x_len"], a["off"], a["ln"], a["S"], a["max_len"], a["sr"], a["ws"],
                                                    a["ws_bytes"], a["loud"], a["cnt"], None))({**ok, **k})
    for name in ("x", "off", "ln", "ws", "loud"):
        refused(call(**{name: None}), "null")
    refused(call(S=0), "S must")
    refused(call(S=-1), "S must")
    refused(call(x_len=0), "x_len")
    refused(call(max_len=0), "max_len")
    refused(call(sr=999), "sr must")
    refused(call(sr=384001), "sr must")
    refused(call(sr=3363, ws_bytes=1 << 30), "stable")           # the shelf's centre frequency above sr / 2
    refused(call(ws_bytes=need - 1), "workspace")
    refused(call(max_len=320000 + 3200), "workspace")            # one hop more needs more
    refused(call(x=x + 2), "misaligned")
    refused(call(off=off + 4), "misaligned")
    refused(call(ln=ln + 4), "misaligned")
    refused(call(ws=ws + 4), "misaligned")
    refused(call(loud=loud + 4), "misaligned")
    refused(call(cnt=cnt + 2), "misaligned")
    # the workspace query refuses what the call refuses, with -1
    for bad in ((0, 320000, 32000), (4, 0, 32000), (4, 320000, 999), (4, 320000, 384001), (4, 320000, 3363)):
        assert lib.bsed_loudness_ws_bytes(*bad) == -1 and b"bsed_loudness_ws_bytes" in lib.bsed_last_error()
    # its size: 8 bytes per segment and whole hop of the longest effective length (a short segment is tiled to < 1 s)
    assert lib.bsed_loudness_ws_bytes(1, 1, 32000) == 8 * 5
    assert lib.bsed_loudness_ws_bytes(3, 16000, 32000) == 8 * 3 * 10
    assert lib.bsed_loudness_ws_bytes(2, 11025 * 3, 11025) == 8 * 2 * 30


@pytest.mark.parametrize("sr", [8000, 11025, 16000, 22050, 32000, 44100, 48000, 96000])
def test_kweight_coefs_agree_with_the_restatement(sr):
    out = (ctypes.c_double * 10)()
    assert L.lib().bsed_kweight_coefs(sr, out) == 0
    assert np.abs(np.array(out[:]) - lr.coefs10(sr)).max() <= 1e-12


def test_kweight_coefs_refuses_bad_arguments():
    lib = L.lib()
    out = (ctypes.c_double * 10)()
    assert lib.bsed_kweight_coefs(32000, None) == -1 and b"null" in lib.bsed_last_error()
    for sr in (999, 384001, 0, -32000):
        assert lib.bsed_kweight_coefs(sr, out) == -1 and b"sr must" in lib.bsed_last_error()


# ---- plans levelled by LUFS --------------------------------------------------------------------------------------------
LENGTH = [3000, 40000, 16000, 400000, 8000, 500000, 320000]
CLASS = [0, 1, 2, 2, 3, -1, -1]
RMS = [0.1, 0.2, 0.05, 0.3, 0.0, 0.01, 0.02]
LUFS = [-23.5, -17.25, -30.125, -12.0, -math.inf, -44.75, -math.inf]     # item 4 and background 6 are silent


def _banks():
    return (synth.SoundBank.layout(BIRD_LIST, LENGTH, CLASS, RMS), synth.SoundBank.layout(BIRD_LIST, LENGTH, CLASS, RMS, 32000, LUFS))


_TABLES = ("bg_off", "bg_len", "bg_phase", "n_ev", "src", "on", "len", "inv_fade", "cls", "on_f", "off_f", "onset_s", "offset_s")


def _items(bank, plan):
    """(B, K) bank item of every event slot; (B,) of every background"""
    return np.searchsorted(bank.offset, plan.src, side="right") - 1, np.searchsorted(bank.offset, plan.bg_off, side="right") - 1


def test_lufs_plan_differs_from_the_rms_plan_in_the_gains_alone():
    plain, bank = _banks()
    assert plain.lufs is None and bank.lufs.dtype == np.float64 and np.array_equal(bank.rms, plain.rms)
    kw = dict(clip_seconds=10.0, n_events=(2, 6), snr_db=(6.0, 30.0))
    rms_plan = synth.plan_soundscapes(bank, 32, np.random.default_rng(11), **kw)
    lufs_plan = synth.plan_soundscapes(bank, 32, np.random.default_rng(11), loudness="lufs", **kw).validate(bank)
    for name in _TABLES:
        assert np.array_equal(getattr(rms_plan, name), getattr(lufs_plan, name)), name
    used = lufs_plan.used
    assert used.sum() > 60 and not np.array_equal(rms_plan.g[used], lufs_plan.g[used])
    # the SNR each plan implies is the same draw: recover it from either gain
    item, bg = _items(bank, lufs_plan)
    audible = used & np.isfinite(bank.lufs[item])
    assert audible.sum() > 40 and (used & ~audible).any() and (lufs_plan.g[used & ~audible] == 0).all()
    snr_rms = 20.0 * np.log10(rms_plan.g[audible].astype(np.float64) * bank.rms[item[audible]]) + 55.0
    snr_lufs = 20.0 * np.log10(lufs_plan.g[audible].astype(np.float64)) + bank.lufs[item[audible]] + 55.0
    assert np.abs(snr_rms - snr_lufs).max() <= 1e-5 and snr_lufs.min() >= 6.0 - 1e-5 and snr_lufs.max() <= 30.0 + 1e-5
    # backgrounds: 10^((ref_db - lufs) / 20) in float64, rounded to float32; the silent one gets 0
    want = np.where(np.isneginf(bank.lufs[bg]), 0.0, 10.0 ** ((-55.0 - np.where(np.isneginf(bank.lufs[bg]), 0.0, bank.lufs[bg])) / 20.0))
    assert np.array_equal(lufs_plan.bg_gain, want.astype(np.float32)) and lufs_plan.bg_gain.dtype == np.float32
    assert (lufs_plan.bg_gain[bg == 6] == 0).all() and (bg == 6).any() and (lufs_plan.bg_gain[bg == 5] > 0).all() and (bg == 5).any()
    # a default call on the bank with lufs is today's plan, bit for bit, and equals the plan of the bank without it
    default = synth.plan_soundscapes(plain, 32, np.random.default_rng(11), **kw)
    for name in _TABLES + ("g", "bg_gain"):
        assert np.array_equal(getattr(default, name), getattr(rms_plan, name)), name
    want_g = (10.0 ** (-55.0 / 20.0) / np.array(RMS)[5]).astype(np.float32)
    assert (default.bg_gain[bg == 5] == want_g).all()            # the RMS rule, restated


def test_lufs_gains_are_the_float64_formula_rounded_to_float32():
    _, bank = _banks()
    for ref_db, snr in ((-55.0, 12.0), (-30.0, 0.0), (-41.5, 23.75)):
        plan = synth.plan_soundscapes(bank, 16, np.random.default_rng(5), n_events=(3, 6), snr_db=(snr, snr), ref_db=ref_db,
                                      loudness="lufs")
        item, bg = _items(bank, plan)
        lufs = bank.lufs[item]
        want = np.where(np.isneginf(lufs), 0.0, 10.0 ** ((ref_db + snr - np.where(np.isneginf(lufs), 0.0, lufs)) / 20.0))
        used = plan.used
        assert plan.g.dtype == np.float32 and np.array_equal(plan.g[used], want.astype(np.float32)[used])
        assert (plan.g[used][np.isneginf(lufs[used])] == 0).all() and np.isneginf(lufs[used]).any()
        one = np.float32(10.0 ** ((ref_db + snr - (-17.25)) / 20.0))                 # item 1, by hand
        assert (plan.g[used & (item == 1)] == one).all() and (used & (item == 1)).any()


def test_lufs_plan_needs_a_bank_with_lufs_and_a_known_mode():
    plain, bank = _banks()
    with pytest.raises(L.BsedError, match="lufs"):
        synth.plan_soundscapes(plain, 2, np.random.default_rng(0), loudness="lufs")
    with pytest.raises(L.BsedError, match="loudness"):
        synth.plan_soundscapes(bank, 2, np.random.default_rng(0), loudness="peak")
    with pytest.raises(L.BsedError, match="loudness"):
        synth.SoundBank.layout(BIRD_LIST, LENGTH, CLASS, RMS, 32000, LUFS[:-1])        # one value per item
    with pytest.raises(L.BsedError, match="loudness"):
        synth.SoundBank.layout(BIRD_LIST, LENGTH, CLASS, RMS, 32000, [math.nan] * 7)
    with pytest.raises(L.BsedError, match="loudness"):
        synth.SoundBank([], [], BIRD_LIST, loudness="peak")
