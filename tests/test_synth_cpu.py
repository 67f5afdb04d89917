"""Host side of the soundscape synthesis (bsed_amd.synth): the sampler, the plan's validation, annotations and frame
tables, the argument checks of the two entry points (no device is touched) and the float64 reference against itself."""
import json
import os

import numpy as np
import pytest

import synth_reference as sr_
from bsed_amd import _lib as L
from bsed_amd import synth
from bsed_amd.labels import BIRD_LIST, ManyHotEncoder
from bsed_amd.parallel import rank_seed

LABELS = ["EATO", "WOTH", "BCCH", "BTNW"]
SR = 32000


def _bank(sr=SR):
    # snippets of 0.05 s .. 12 s (longer than a clip), BTNW without any; two backgrounds, one silent
    length = [1600, 9000, 40000, 384000, 64000, 12345, 320000, 100000]
    cls = [0, 0, 1, 1, 2, 2, -1, -1]
    rms = [0.1, 0.2, 0.05, 0.3, 0.01, 0.5, 0.02, 0.0]
    return synth.SoundBank.layout(LABELS, length, cls, rms, sr=sr)


def _plan(bank, B, seed, step, **kw):
    return synth.plan_soundscapes(bank, B, np.random.default_rng(rank_seed(seed, step, 0)), **kw)


_ARRAYS = ("bg_off", "bg_len", "bg_phase", "bg_gain", "n_ev", "src", "on", "len", "g", "inv_fade", "cls", "on_f", "off_f",
           "onset_s", "offset_s")


def test_same_seed_same_plan_and_another_step_another_plan():
    bank = _bank()
    a, b, c = _plan(bank, 16, 7, 3), _plan(bank, 16, 7, 3), _plan(bank, 16, 7, 4)
    for name in _ARRAYS:
        assert np.array_equal(getattr(a, name), getattr(b, name)), name
    assert not (np.array_equal(a.on, c.on) and np.array_equal(a.src, c.src))
    np.random.seed(0)                                    # the global generator plays no part
    d = _plan(bank, 16, 7, 3)
    assert np.array_equal(a.on, d.on) and np.array_equal(a.g, d.g)


@pytest.mark.parametrize("max_polyphony", [1, 2, 4])
def test_plans_are_valid_polyphony_is_bounded_and_events_are_long_enough(max_polyphony):
    bank = _bank()
    min_s = 0.2
    plan = _plan(bank, 48, 11, max_polyphony, max_polyphony=max_polyphony, n_events=(1, 9), min_event_seconds=min_s)
    assert plan.validate(bank) is plan
    assert plan.n == 10 * SR and plan.K == synth.MAX_EVENTS and (plan.n_ev >= 1).all()
    ends = bank.offset + bank.length
    for b in range(plan.B):
        active = np.zeros(plan.n + 1, np.int64)
        for k in range(int(plan.n_ev[b])):
            on, ln = int(plan.on[b, k]), int(plan.len[b, k])
            active[on] += 1
            active[on + ln] -= 1
            item = int(np.searchsorted(bank.offset, plan.src[b, k], side="right") - 1)
            assert bank.cls[item] == plan.cls[b, k] and plan.src[b, k] + ln <= ends[item]
            assert ln >= min(int(np.ceil(min_s * SR)), int(bank.length[item]))
            assert ln == min(int(bank.length[item]), plan.n)            # snippets are used whole, or cut to the clip
            want_g = 10.0 ** ((-55.0 + 6.0) / 20.0) / bank.rms[item], 10.0 ** ((-55.0 + 30.0) / 20.0) / bank.rms[item]
            assert want_g[0] * (1 - 1e-6) <= plan.g[b, k] <= want_g[1] * (1 + 1e-6)
        assert np.cumsum(active).max() <= max_polyphony
    assert (plan.cls[plan.used] != LABELS.index("BTNW")).all()          # a label without snippets is never drawn
    silent = plan.bg_off == bank.offset[7]
    assert silent.any() and (~silent).any()
    assert (plan.bg_gain[silent] == 0).all()                            # a silent background: gain 0, not infinity
    np.testing.assert_allclose(plan.bg_gain[~silent], 10.0 ** (-55.0 / 20.0) / 0.02, rtol=1e-6)
    if max_polyphony == 1:
        assert (plan.n_ev < 9).any()                                    # some draws ran out of redraws and were dropped


def test_no_backgrounds_means_silence_and_bad_arguments_raise():
    bank = synth.SoundBank.layout(LABELS, [1000, 2000], [0, 3], [0.1, 0.1])
    plan = _plan(bank, 4, 1, 0, clip_seconds=1.0)
    assert (plan.bg_len == 0).all() and plan.n == SR
    plan.validate(bank)
    with pytest.raises(L.BsedError):
        synth.plan_soundscapes(bank, 4, np.random.RandomState(0))       # not a Generator
    with pytest.raises(L.BsedError):
        _plan(bank, 4, 1, 0, class_probs=[0, 1, 0, 0])                  # weight on a label without snippets
    with pytest.raises(L.BsedError):
        _plan(bank, 4, 1, 0, clip_seconds=0.1)                          # shorter than min_event_seconds
    with pytest.raises(L.BsedError):
        synth.SoundBank.layout(LABELS, [1000, 0], [0, 1], [0.1, 0.1])   # an empty snippet
    with pytest.raises(L.BsedError):
        synth.SoundBank.layout(LABELS, [1000], [4], [0.1])              # a class outside the labels


def test_co_occurrence_only_places_listed_classes(golden_dir):
    co = json.load(open(os.path.join(golden_dir, "event_occurences_train.json")))
    labels = ["AMCR", "RCKI", "AMGO", "WBNU", "EATO"]                    # EATO has snippets but is not in the table
    bank = synth.SoundBank.layout(labels, [8000, 9000, 10000, 11000, 12000, 64000], [0, 1, 2, 3, 4, -1], [0.1] * 6)
    plan = _plan(bank, 200, 5, 0, co_occurrence=co, max_polyphony=16).validate(bank)
    mains = set()
    for b in range(plan.B):
        names = [labels[c] for c in plan.cls[b, :plan.n_ev[b]]]
        main = names[0]
        mains.add(main)
        assert main in co and 1 <= len(names) <= co[main]["co-occurences"]["max_events"]
        assert set(names[1:]) <= set(co[main]["co-occurences"]["classes"]), (main, names)
    assert mains == set(co)                                             # 200 clips: every main class turns up
    assert (plan.n_ev > 1).any()
    with pytest.raises(L.BsedError):                                    # the table names a class the bank has no snippet of
        _plan(synth.SoundBank.layout(labels, [8000], [0], [0.1]), 4, 5, 0, co_occurrence=co)


def _one_clip(events, n=10 * SR, sr=SR, labels=LABELS):
    """a hand-made one-clip plan of (on, len, label) events"""
    K = max(len(events), 1)
    z = np.zeros((1, K))
    on, ln, cls = z.copy(), np.ones((1, K)), z.copy()
    for k, (a, l, lab) in enumerate(events):
        on[0, k], ln[0, k], cls[0, k] = a, l, labels.index(lab)
    return synth.SoundscapePlan(n, sr, labels, [0], [0], [0], [0.0], [len(events)], z, on, ln, z + 1, z + 1, cls, names=["c"])


def test_annotations_merge_overlapping_same_label_events_only():
    plan = _one_clip([(64000, 32000, "EATO"),        # 2.0 - 3.0
                      (80000, 32000, "EATO"),        # 2.5 - 3.5: overlaps the first
                      (112000, 16000, "WOTH"),       # 3.5 - 4.0: touches the merged EATO, another label
                      (160000, 16000, "EATO"),       # 5.0 - 5.5: apart
                      (0, 3200, "WOTH")])            # 0.0 - 0.1
    raw = plan.annotations(merge_same_label=False)
    assert list(raw.columns) == ["filename", "onset", "offset", "event_label"] and len(raw) == 5
    assert raw["onset"].tolist() == [2.0, 2.5, 3.5, 5.0, 0.0] and set(raw["filename"]) == {"c.wav"}
    got = plan.annotations(merge_same_label=True)
    rows = sorted(zip(got["onset"], got["offset"], got["event_label"]))
    assert rows == [(0.0, 0.1, "WOTH"), (2.0, 3.5, "EATO"), (3.5, 4.0, "WOTH"), (5.0, 5.5, "EATO")]


def test_validate_refuses_what_the_kernel_must_not_be_given():
    bank = _bank()
    ok = dict(on=1000, ln=1600, src=0, g=1.0, f=0.5)

    def plan_with(K=1, n_ev=1, bg_len=0, bg_off=0, **kw):
        v = dict(ok, **kw)
        full = lambda x: np.full((1, K), x)
        return synth.SoundscapePlan(SR, SR, LABELS, [bg_off], [bg_len], [0], [1.0], [n_ev], full(v["src"]), full(v["on"]),
                                    full(v["ln"]), full(v["g"]), full(v["f"]), full(0))
    plan_with().validate(bank)
    plan_with(K=16, n_ev=16).validate(bank)
    plan_with(bg_len=320000, bg_off=int(bank.offset[6])).validate(bank)
    for defect in (dict(on=SR - 1599), dict(on=-1), dict(ln=1601), dict(src=1), dict(ln=0), dict(g=-0.5), dict(f=0.0),
                   dict(f=1.5), dict(n_ev=2), dict(K=17, n_ev=1), dict(bg_len=320001, bg_off=int(bank.offset[6])),
                   dict(src=int(bank.total_samples) - 100)):
        with pytest.raises(L.BsedError, match="SoundscapePlan"):
            plan_with(**defect).validate(bank)


@pytest.mark.parametrize("sr", sorted(sr_.BOUNDARY_ONSETS))
def test_frames_are_the_encoders_at_the_onsets_where_integer_division_differs(sr):
    enc = ManyHotEncoder(BIRD_LIST, n_frames=313 if sr == 32000 else 216, sr=sr)
    onsets = [s + d for s in sr_.BOUNDARY_ONSETS[sr] for d in (-1, 0, 1)]
    plan = _one_clip([(s, 5000, "EATO") for s in onsets], sr=sr)
    differ = 0
    for k, s in enumerate(onsets):
        assert plan.onset_s[0, k] == s / sr and plan.offset_s[0, k] == (s + 5000) / sr
        assert plan.on_f[0, k] == enc.frame(plan.onset_s[0, k]), (sr, s)
        assert plan.off_f[0, k] == enc.frame(plan.offset_s[0, k]), (sr, s)
        differ += int(plan.on_f[0, k] != s // (255 * 4))
    assert differ >= len(sr_.BOUNDARY_ONSETS[sr])      # these are the onsets at which the integer shortcut is wrong


def test_frame_tables_give_the_recorded_frames_of_the_reference_encoder(golden_dir):
    cases = json.load(open(os.path.join(golden_dir, "labels_kat.json")))
    for c in cases:
        ev = [(round(a * SR), round(b * SR) - round(a * SR), lab) for a, b, lab in c["events"]]
        plan = _one_clip(ev, labels=BIRD_LIST)
        assert plan.onset_s[0, :len(ev)].tolist() == [e[0] for e in c["events"]]      # whole milliseconds: exact at 32 kHz
        y = np.zeros((313, len(BIRD_LIST)))
        for k in range(len(ev)):
            y[plan.on_f[0, k]:plan.off_f[0, k], plan.cls[0, k]] = 1
        assert float(y.sum()) == c["sum"] and y.sum(0).tolist() == c["col_sums"]
        for lab, (first, last) in c["first_last"].items():
            col = y[:, BIRD_LIST.index(lab)].nonzero()[0]
            assert (int(col.min()), int(col.max()) + 1) == (first, last)


def test_entry_points_refuse_bad_arguments_before_any_launch():
    lib = L.lib()
    assert lib.bsed_abi_version() >= 9
    assert L.CONSTANTS["BSED_SYNTH_MAX_EVENTS"] == 16 and "BsedSynth" not in "".join(L.STRUCTS)
    d = 0x1000                                           # dummy non-null pointers: never dereferenced on the host

    def mix(bank=d, first_table=d, last_table=d, B=3, n=20011, K=16, out=d):
        return lib.bsed_synth_mix(bank, 1000, first_table, d, d, d, d, d, d, d, d, last_table, B, n, K, out, None)

    def tgt(n_ev=d, B=3, K=16, T=313, C=20, strong=d, weak=d):
        return lib.bsed_synth_targets(n_ev, d, d, d, B, K, T, C, strong, weak, None)
    for call, prefix in ((mix, "bsed_synth_mix:"), (tgt, "bsed_synth_targets:")):
        defects = [dict(K=17), dict(K=-1), dict(B=0)]
        defects += [dict(bank=None), dict(first_table=None), dict(last_table=None), dict(out=None), dict(out=d + 4),
                    dict(n=0)] if call is mix else [dict(n_ev=None), dict(strong=None), dict(weak=None), dict(strong=d + 2),
                                                    dict(T=0), dict(C=0)]
        for defect in defects:
            rc = call(**defect)
            msg = lib.bsed_last_error().decode()
            assert rc == -1 and msg.startswith(prefix), (prefix, defect, rc, msg)
    assert b"16-byte" in (mix(out=d + 4), lib.bsed_last_error())[1]


def test_reference_reproduces_a_shifted_snippet():
    rng = np.random.default_rng(0)
    bank = (0.3 * rng.standard_normal(5000)).astype(np.float32)
    n, on, ln, src = 4001, 1234, 777, 2001
    z = np.zeros((1, 1))
    plan = synth.SoundscapePlan(n, SR, LABELS, [0], [0], [0], [0.0], [1], z + src, z + on, z + ln, z + 1, z + 1, z)
    ref, S, K = sr_.mix_ref(bank, plan)
    want = np.zeros(n)
    want[on:on + ln] = bank[src:src + ln]
    assert np.array_equal(ref[0], want) and np.array_equal(S[0], np.abs(want))
    assert K[0].sum() == ln and K[0, on] == 1 and K[0, on - 1] == 0 and K[0, on + ln] == 0
    assert (sr_.fade_weight(1000, 1.0) == 1).all()
    w = sr_.fade_weight(1000, 1.0 / 320.0)
    assert w[0] == np.float32(1.0 / 320.0) and w[-1] == w[0] and (w[319:681] == 1).all() and w[318] < 1 and w[681] < 1
    # a wrapping background alone
    plan = synth.SoundscapePlan(10, SR, LABELS, [100], [4], [3], [2.0], [0], z, z, z + 1, z, z + 1, z)
    ref, S, K = sr_.mix_ref(bank, plan)
    assert np.array_equal(ref[0], 2.0 * bank[100 + (3 + np.arange(10)) % 4].astype(np.float64)) and K.sum() == 0
